"""CPU-only checks of the truncated signed distance volumes (include/ctd_hip_tsdf.h: ctd_tsdf_integrate_f32,
ctd_tsdf_surface_points_f32, ctd_tsdf_raycast_f32; torchext.tsdf_volume, tsdf_integrate, tsdf_surface_points,
tsdf_raycast): the rules' sentences (the header against its ctypes table and the built library:
tests/test_abi_and_host.py), argument validation before any HIP call and its precedence, the workspace query, the Python surface, and the restatement
tests/tsdf_ref.py against the truth of its scenes.

Measured on the restatement.  Scenes of tests/fusion_ref.py: B=1, V=4, 48 x 64, a 48^3 grid over 1.6 m around
(0.1, 0, 2.2), trunc = 4 voxels; the tests run seed 5 (seeds 5 and 6 for "noisy") and pin 2 x its values.
  integrate    "plane", every pixel valid: |tsdf * trunc - the mean over the views of the true signed distance along the
               view's z| is at most 1.76e-3 (seeds 6, 7: 1.77e-3, 1.64e-3) against the bound 2.85e-3 (3.12e-3, 3.64e-3) that
               test_integrate_measures_the_distance_along_the_view derives from the pixel rounding; the weight equals the
               number of views that see the voxel at every voxel whose membership does not hang on the rounding (84 % of
               the voxels; 43 % of those are seen by no view).
  plane        the largest distance of a surface point to the plane is 1.60e-3 (seeds 6, 7: 2.15e-3, 1.48e-3; the
               numpy prototype of the rules gave 1.9e-3 on its grid).  Asserted: 2.0e-3, the bound the rules were
               accepted with, which is below 2 x 1.60e-3.  93 % of the points have a normal (the others lie at the border
               of the observed band); its largest angle to the plane's is 2.15 degrees (seeds 6, 7: 2.44, 1.67), pinned
               at 4.30.
  clean        the share of points farther than one voxel from both planes is 3.11 % (seeds 6, 7: 2.21 %, 3.72 %; the
               prototype had 3.5 %): the edge artefacts where the patch occludes the plane.  Capped at 6.22 %.
  noisy        with valid = keep of the consistency rule (max_rel 0.01, min_views 1) the median distance of the surface
               points to the true surfaces is 1.88e-3 / 1.89e-3 at seeds 5 / 6, that of the kept per-view points
               3.18e-3 / 3.22e-3: 0.592 / 0.585 of it (asserted <= 0.75).  Without the mask (valid of the scene only) the
               10 % gross outliers bias the volume: 1.67e-2 / 1.66e-2 against 3.58e-3 / 3.66e-3 for the raw points, 4.65 /
               4.53 times WORSE, which is why the documented use is valid=keep.
Corner scene of tests/icp_ref.py: B=1, V=5, 48 x 80, seed 5, views 0..3 integrated at their true poses into a 72 x 48 x 32
grid of 0.032 around (0, 0, 2.35); ray cast at 28 steps of 0.048 from 1.7.
  ray cast     at the pose of view 0 / of view 4 (not integrated): 97.6 % / 97.6 % of the pixels whose true point lies
               inside the grid hit (asserted >= 90 %; at seed 6 view 4 looks past what the four views saw and reaches
               85.6 %, seed 7: 96.5 % / 94.9 %); median |depth - truth| = 0.0107 / 0.0103 voxel (seeds 6, 7: 0.0091 / 0.0097
               and 0.0113 / 0.0114), pinned at 0.0214 voxel; largest 0.14 voxel, at the creases.
  frame-to-model  the volume integrated with valid = keep of the consistency rule (max_rel 0.01), as documented; view 0 =
               its ray cast at the pose of view 4, view 1 = the real view 1 with its pose off by 1 degree / 1 cm; 6 rounds
               of icp_ref.depth_icp: translation error 9.70e-3 -> 3.26e-4, rotation error 1.000 -> 1.78e-2 degrees (seeds
               6, 7: 4.52e-4 / 8.0e-3 and 1.46e-4 / 6.3e-3), pinned at 6.52e-4 and 3.56e-2 degrees.  (keep drops the border
               pixels that no second view confirms, so this cast hits 90.9 % / 89.4 % of the pixels; the ray-cast test
               above integrates every pixel.)
"""
import ctypes
import inspect
import os

import numpy as np
import pytest
import torch

from tests import fusion_ref as fr
from tests import icp_ref as ir
from tests import tsdf_ref as tr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TSDF_HEADER = os.path.join(ROOT, "include", "ctd_hip_tsdf.h")

OK, INVALID_ARG, WORKSPACE, UNSUPPORTED = 0, 1, 2, 3
NAN, INF = float("nan"), float("inf")
F = np.float32

# the scenes of the truth tests; tests/test_tsdf_gpu.py uses the corner model and its pins
PLANE_SHAPE, PLANE_SEED, PLANE_GRID = (1, 4, 48, 64), 5, (48, 1.6, (0.1, 0.0, 2.2))
MAX_PLANE_DIST = 2.0e-3                                          # the bound of the rules; below 2 x the measured 1.60e-3
MAX_PLANE_NORMAL_DEG = 2 * 2.15
MAX_CLEAN_FAR_SHARE = 2 * 0.0311
MAX_NOISY_RATIO = 0.75
CORNER_SHAPE, CORNER_SEED = (1, 5, 48, 80), 5
CORNER_DIMS, CORNER_VOXEL, CORNER_CENTRE = (72, 48, 32), 0.032, (0.0, 0.0, 2.35)
CAST = dict(d_min=1.7, step=0.048, n_steps=28)
MIN_HIT_SHARE = 0.90
MAX_CAST_MEDIAN_VOXELS = 2 * 0.0107
F2M_ITERS, MAX_F2M_T_ERR, MAX_F2M_ROT_ERR_DEG = 6, 2 * 3.26e-4, 2 * 1.78e-2


@pytest.fixture(scope="module")
def L():
    from connecting_the_dots_amd import _lib
    return _lib.lib()


@pytest.fixture(scope="module")
def te():
    from connecting_the_dots_amd import torchext
    return torchext


# ---------------------------------------------------------------------------------------------------------------------
# 1. the header (header == table == exports: tests/test_abi_and_host.py, for every header)
# ---------------------------------------------------------------------------------------------------------------------
def test_the_header_states_the_rules():
    text = " ".join(open(TSDF_HEADER).read().replace("*", " ").split())
    for phrase in ("X_c = origin[b][c] + voxel (float)index_c",
                   "tsdf is never read where weight == 0",
                   "visit the views v = 0 .. V-1 in ascending order",
                   "Skip the view unless uvd2 > 0",
                   "xs = floorf(uvd0/uvd2 + 0.5f) and ys = floorf(uvd1/uvd2 + 0.5f)",
                   "sdf = depth[q] ray[q][2] - S2. Skip the view if sdf < -trunc",
                   "obs = fminf(1, sdf/trunc)",
                   "If weight == 0 then tsdf = obs, else tsdf = (tsdf weight + obs)/(weight + 1)",
                   "weight = fminf(weight + 1, max_weight)",
                   "a voxel that no view touched is not stored",
                   "A voxel is usable when weight >= min_weight and |tsdf| < 1",
                   "both are usable and (T_a < 0) != (T_n < 0)",
                   "component c increased by voxel (T_a / (T_a - T_n))",
                   "src = (((b nz + k) ny + j) nx + i) 3 + c",
                   "the smaller |T| (a on a tie)",
                   "With points == NULL it only counts",
                   "d_n = d_min + step (float)n for n = 0 .. n_steps-1",
                   "g_c = (X_c - origin_c)/voxel, i0_c = floorf(g_c), f_c = g_c - i0_c",
                   "along x first (a = T0 + fx (T1 - T0) for the four x edges), then y, then z",
                   "the depth is d_{n-1} + step (T_{n-1}/(T_{n-1} - T_n))",
                   "Either way the ray stops",
                   "No call uses atomics; the same bits come out on every run"):
        assert phrase in text, phrase


# ---------------------------------------------------------------------------------------------------------------------
# 2. validation
# ---------------------------------------------------------------------------------------------------------------------
class _Bufs:
    """host buffers standing in for device pointers, 4 KiB apart and 256-byte aligned: validation must reject before any
    of them is ever dereferenced"""

    def __init__(self, names, slot=4096):
        self.raw = ctypes.create_string_buffer(slot * (len(names) + 1))
        base = (ctypes.addressof(self.raw) + 255) // 256 * 256
        self.ptr = {n: base + i * slot for i, n in enumerate(names)}


B, NX, NY, NZ, V, H, W = 2, 3, 4, 5, 3, 4, 5                       # 120 voxels, 120 pixels: every buffer fits a 4 KiB slot
GRID = dict(B=B, nx=NX, ny=NY, nz=NZ)
BIG_GRID = dict(B=1 << 20, nx=2048, ny=1, nz=1)                    # B * nx * ny * nz = 2^31
BIG_IMAGE = dict(B=1 << 11, V=1, H=1 << 10, W=1 << 10)             # B * V * H * W = 2^31 (the grid: 2^11 * 60 voxels)
BIG_SIDE = dict(H=(1 << 24) + 1, W=1)                              # H > 2^24
BAD_POSITIVE = (0.0, -1.0, NAN, INF, -INF)                         # not finite and > 0


def test_integrate_rejections_need_no_gpu(L):
    names = ["tsdf", "weight", "origin", "depth", "valid", "ray", "K", "R", "t"]
    bufs = _Bufs(names)

    def call(voxel=0.1, trunc=0.4, max_weight=64.0, B=B, nx=NX, ny=NY, nz=NZ, V=V, H=H, W=W, **ptrs):
        p = dict(bufs.ptr, **ptrs)
        return L.ctd_tsdf_integrate_f32(p["tsdf"], p["weight"], p["origin"], voxel, p["depth"], p["valid"], p["ray"], p["K"],
                                        p["R"], p["t"], trunc, max_weight, B, nx, ny, nz, V, H, W, -1, None)

    for kw in (dict(nx=0), dict(ny=0), dict(nz=-3), dict(V=0), dict(H=0), dict(W=-2), dict(B=-1), dict(V=65, H=1, W=1)):
        assert call(**kw) == INVALID_ARG, kw
    for bad in BAD_POSITIVE:
        assert call(voxel=bad) == INVALID_ARG and call(trunc=bad) == INVALID_ARG, bad
    for bad in (0.5, 0.0, -1.0, NAN, INF):
        assert call(max_weight=bad) == INVALID_ARG, bad
    for k in names:
        if k != "valid":                                            # (valid may be NULL)
            assert call(**{k: None}) == INVALID_ARG, k
    for kw in (dict(nx=2049), dict(ny=2049), dict(nz=2049), BIG_GRID, BIG_IMAGE, BIG_SIDE, dict(H=1, W=(1 << 24) + 1),
               dict(B=8192, nx=1, ny=1, nz=2048, V=1, H=1, W=1)):    # the last: 2^24 tiles of one voxel each
        assert call(**kw) == UNSUPPORTED, kw
    assert call(B=8191, nx=1, ny=1, nz=2048, V=1, H=1, W=1, tsdf=None) == INVALID_ARG   # (one tile fewer gets past the sizes)
    for out in ("tsdf", "weight"):
        for other in names:
            if other != out:
                assert call(**{out: bufs.ptr[other]}) == INVALID_ARG, (out, other)
    assert call(weight=bufs.ptr["tsdf"] + 4 * B * NX * NY * NZ - 4) == INVALID_ARG
    # precedence: INVALID_ARG, then UNSUPPORTED, then the overlaps
    assert call(trunc=NAN, **BIG_GRID) == INVALID_ARG
    assert call(tsdf=None, **BIG_GRID) == INVALID_ARG
    assert call(V=65, nx=2049) == INVALID_ARG
    assert call(weight=bufs.ptr["tsdf"], **BIG_GRID) == UNSUPPORTED
    # no tracks: nothing to do, nothing touched; NULL required pointers are rejected all the same
    assert call(B=0) == OK
    assert call(B=0, valid=None, max_weight=1.0) == OK
    assert call(B=0, voxel=0.0) == INVALID_ARG
    for k in names:
        if k != "valid":
            assert call(B=0, **{k: None}) == INVALID_ARG, k


def test_surface_points_rejections_need_no_gpu(L):
    nws = L.ctd_tsdf_surface_workspace_bytes(B, NX, NY, NZ)
    assert nws == 256 + 256                                         # 120 flag bytes and 2 + 1 offsets, each rounded up to 256
    names = ["tsdf", "weight", "origin", "points", "normals", "src", "n_per_track", "ws"]
    bufs = _Bufs(names)

    def call(voxel=0.1, min_weight=1.0, capacity=100, B=B, nx=NX, ny=NY, nz=NZ, nbytes=None, **ptrs):
        p = dict(bufs.ptr, **ptrs)
        return L.ctd_tsdf_surface_points_f32(p["tsdf"], p["weight"], p["origin"], voxel, min_weight, p["points"], p["normals"],
                                             p["src"], p["n_per_track"], capacity, B, nx, ny, nz, p["ws"],
                                             nws if nbytes is None else nbytes, -1, None)

    for kw in (dict(nx=0), dict(ny=-1), dict(nz=0), dict(B=-1), dict(capacity=-1), dict(src=None)):
        assert call(**kw) == INVALID_ARG, kw
    for bad in BAD_POSITIVE:
        assert call(voxel=bad) == INVALID_ARG and call(min_weight=bad) == INVALID_ARG, bad
    for k in ("tsdf", "weight", "origin", "n_per_track"):
        assert call(**{k: None}) == INVALID_ARG, k
    for kw in (dict(nx=2049), dict(ny=2049), dict(nz=2049), BIG_GRID, dict(B=1, nx=1024, ny=1024, nz=1024),   # 3 * 2^30 points
               dict(B=1 << 24, nx=1, ny=1, nz=1)):                                                          # 2^24 workgroups
        assert call(**kw) == UNSUPPORTED, kw
    for out in ("points", "normals", "src", "n_per_track", "ws"):
        for other in names:
            if other != out:
                assert call(**{out: bufs.ptr[other]}) == INVALID_ARG, (out, other)
    assert call(points=bufs.ptr["tsdf"] + 476) == INVALID_ARG       # the last float of tsdf
    assert call(ws=None) == WORKSPACE                               # workspace missing, short, misaligned
    assert call(nbytes=nws - 1) == WORKSPACE
    assert call(nbytes=0) == WORKSPACE
    assert call(ws=bufs.ptr["ws"] + 8) == WORKSPACE
    # precedence: INVALID_ARG, then UNSUPPORTED, then the overlaps, then WORKSPACE
    assert call(ws=None, **BIG_GRID) == UNSUPPORTED
    assert call(ws=None, min_weight=NAN, **BIG_GRID) == INVALID_ARG
    assert call(ws=None, n_per_track=None, **BIG_GRID) == INVALID_ARG
    assert call(ws=None, points=bufs.ptr["weight"]) == INVALID_ARG
    # counting only: points NULL, and then normals, src and capacity are not looked at
    assert call(points=None, normals=None, src=None, capacity=-5, nbytes=0) == WORKSPACE
    assert call(points=None, normals=bufs.ptr["tsdf"], src=bufs.ptr["weight"], nbytes=0) == WORKSPACE
    assert call(normals=None, nbytes=0) == WORKSPACE                # normals are optional
    # no tracks: nothing to do, nothing touched, no workspace needed
    assert call(B=0, ws=None, nbytes=0) == OK
    assert call(B=0, ws=None, nbytes=0, points=None, normals=None, src=None) == OK
    assert call(B=0, ws=None, nbytes=0, voxel=-1.0) == INVALID_ARG
    assert call(B=0, ws=None, nbytes=0, tsdf=None) == INVALID_ARG
    assert call(B=0, ws=None, nbytes=0, n_per_track=None) == INVALID_ARG


def test_surface_workspace_query(L):
    for b, nx, ny, nz in [(4, 256, 256, 256), (1, 2, 2, 2), (2, 33, 18, 21), (2, 64, 5, 7), (1, 1, 1, 1), (3, 256, 1, 1),
                          (3, 257, 1, 1)]:
        nvox = nx * ny * nz
        chunks = (nvox + 255) // 256
        want = (b * nvox + 255) // 256 * 256 + (4 * (b * chunks + 1) + 255) // 256 * 256
        assert L.ctd_tsdf_surface_workspace_bytes(b, nx, ny, nz) == want > 0
    for args in ((0, 8, 8, 8), (-1, 8, 8, 8), (1, 0, 8, 8), (1, 8, -1, 8), (1, 8, 8, 0), (1, 2049, 1, 1), (1 << 20, 2048, 1, 1),
                 (1, 1024, 1024, 1024), (1 << 24, 1, 1, 1)):
        assert L.ctd_tsdf_surface_workspace_bytes(*args) == 0, args


def test_raycast_rejections_need_no_gpu(L):
    names = ["tsdf", "weight", "origin", "ray", "R", "t", "depth"]
    bufs = _Bufs(names)

    def call(voxel=0.1, d_min=0.5, step=0.05, n_steps=32, min_weight=1.0, B=B, nx=NX, ny=NY, nz=NZ, V=V, H=H, W=W, **ptrs):
        p = dict(bufs.ptr, **ptrs)
        return L.ctd_tsdf_raycast_f32(p["tsdf"], p["weight"], p["origin"], voxel, p["ray"], p["R"], p["t"], d_min, step, n_steps,
                                      min_weight, p["depth"], B, nx, ny, nz, V, H, W, -1, None)

    for kw in (dict(nx=0), dict(ny=0), dict(nz=-3), dict(V=0), dict(H=0), dict(W=-2), dict(B=-1), dict(V=65, H=1, W=1),
               dict(n_steps=0), dict(n_steps=-4)):
        assert call(**kw) == INVALID_ARG, kw
    for bad in BAD_POSITIVE:
        assert call(voxel=bad) == INVALID_ARG and call(step=bad) == INVALID_ARG and call(min_weight=bad) == INVALID_ARG, bad
    for bad in (-1e-3, NAN, INF, -INF):
        assert call(d_min=bad) == INVALID_ARG, bad
    for k in names:
        assert call(**{k: None}) == INVALID_ARG, k
    for kw in (dict(nx=2049), dict(ny=2049), dict(nz=2049), BIG_GRID, BIG_IMAGE, BIG_SIDE, dict(H=1, W=(1 << 24) + 1),
               dict(B=1 << 18, V=64, H=1, W=1, nx=1, ny=1, nz=1)):     # the last: 2^24 views of one tile each
        assert call(**kw) == UNSUPPORTED, kw
    for other in names[:-1]:
        assert call(depth=bufs.ptr[other]) == INVALID_ARG, other
    assert call(depth=bufs.ptr["ray"] + 8) == INVALID_ARG
    # precedence: INVALID_ARG, then UNSUPPORTED, then the overlaps
    assert call(step=NAN, **BIG_GRID) == INVALID_ARG
    assert call(depth=None, **BIG_IMAGE) == INVALID_ARG
    assert call(depth=bufs.ptr["tsdf"], **BIG_IMAGE) == UNSUPPORTED
    # no tracks: nothing to do, nothing touched; d_min == 0 is fine
    assert call(B=0) == OK
    assert call(B=0, d_min=0.0, n_steps=1) == OK
    assert call(B=0, n_steps=0) == INVALID_ARG
    for k in names:
        assert call(B=0, **{k: None}) == INVALID_ARG, k


# ---------------------------------------------------------------------------------------------------------------------
# 3. the Python surface
# ---------------------------------------------------------------------------------------------------------------------
def test_python_signatures_and_docstrings(te):
    def params(fn):
        return [(k, p.default) for k, p in inspect.signature(fn).parameters.items()]

    E = inspect.Parameter.empty
    assert params(te.tsdf_volume) == [("B", E), ("nx", E), ("ny", E), ("nz", E), ("device", "cuda")]
    assert params(te.tsdf_integrate) == [("tsdf", E), ("weight", E), ("origin", E), ("voxel", E), ("depth", E), ("ray", E),
                                         ("K", E), ("R", E), ("t", E), ("valid", None), ("trunc", None), ("max_weight", 64.0)]
    assert params(te.tsdf_surface_points) == [("tsdf", E), ("weight", E), ("origin", E), ("voxel", E), ("min_weight", 1.0),
                                              ("return_normals", False)]
    assert params(te.tsdf_raycast) == [("tsdf", E), ("weight", E), ("origin", E), ("voxel", E), ("ray", E), ("R", E), ("t", E),
                                       ("H", E), ("W", E), ("d_min", E), ("step", E), ("n_steps", E), ("min_weight", 1.0)]
    for fn in (te.tsdf_integrate, te.tsdf_surface_points, te.tsdf_raycast):
        assert "obs = min(1, sdf / trunc)" in fn.__doc__ and "weight >= min_weight and |tsdf| < 1" in fn.__doc__, fn.__name__
        assert "the same bits on every run" in fn.__doc__
    assert "trunc=None stands for 4 * voxel" in te.tsdf_integrate.__doc__
    assert "`keep` of `depth_consistency` as\n    `valid`" in te.tsdf_integrate.__doc__
    assert "one synchronisation" in te.tsdf_surface_points.__doc__
    assert "depth_icp" in te.tsdf_raycast.__doc__ and "disparity_band_window" in te.tsdf_raycast.__doc__


def test_python_surface_errors(te):
    sc = fr.make_scene("clean", 2, 3, 4, 5, 0)
    depth, ray, K, R, t, valid = [torch.from_numpy(sc[k]) for k in ("depth", "ray", "K", "R", "t", "valid")]
    tsdf, weight = torch.ones(2, 5, 4, 3), torch.zeros(2, 5, 4, 3)
    origin = torch.zeros(2, 3)
    # the numbers, before any tensor is looked at
    for bad in (0.0, -1.0, NAN, INF, "1", None, True):
        with pytest.raises(RuntimeError, match="voxel must be a finite number > 0"):
            te.tsdf_integrate(tsdf, weight, origin, bad, depth, ray, K, R, t)
        with pytest.raises(RuntimeError, match="voxel must be a finite number > 0"):
            te.tsdf_surface_points(tsdf, weight, origin, bad)
        with pytest.raises(RuntimeError, match="min_weight must be a finite number > 0"):
            te.tsdf_surface_points(tsdf, weight, origin, 0.1, min_weight=bad)
        with pytest.raises(RuntimeError, match="step must be a finite number > 0"):
            te.tsdf_raycast(tsdf, weight, origin, 0.1, ray, R, t, 4, 5, 0.5, bad, 8)
        with pytest.raises(RuntimeError, match="min_weight must be a finite number > 0"):
            te.tsdf_raycast(tsdf, weight, origin, 0.1, ray, R, t, 4, 5, 0.5, 0.05, 8, min_weight=bad)
        if bad is not None:                                                # (trunc=None stands for 4 * voxel)
            with pytest.raises(RuntimeError, match="trunc must be a finite number > 0"):
                te.tsdf_integrate(tsdf, weight, origin, 0.1, depth, ray, K, R, t, trunc=bad)
    for bad in (0.5, -1.0, NAN, INF, "1", None, True):
        with pytest.raises(RuntimeError, match="max_weight must be a finite number >= 1"):
            te.tsdf_integrate(tsdf, weight, origin, 0.1, depth, ray, K, R, t, max_weight=bad)
    for bad in (-0.5, NAN, INF, "1", None, True):
        with pytest.raises(RuntimeError, match="d_min must be a finite number >= 0"):
            te.tsdf_raycast(tsdf, weight, origin, 0.1, ray, R, t, 4, 5, bad, 0.05, 8)
    for bad in (0, -1, 2.0, None, True):
        with pytest.raises(RuntimeError, match="n_steps must be an integer >= 1"):
            te.tsdf_raycast(tsdf, weight, origin, 0.1, ray, R, t, 4, 5, 0.5, 0.05, bad)
        with pytest.raises(RuntimeError, match="H must be an integer >= 1"):
            te.tsdf_raycast(tsdf, weight, origin, 0.1, ray, R, t, bad, 5, 0.5, 0.05, 8)
        with pytest.raises(RuntimeError, match="nx must be an integer >= 1"):
            te.tsdf_volume(1, bad, 4, 4)
    with pytest.raises(RuntimeError, match="at most 2048"):
        te.tsdf_volume(1, 4, 2049, 4)
    with pytest.raises(RuntimeError, match="no CPU path"):
        te.tsdf_volume(1, 4, 4, 4, device="cpu")
    # no CPU path: well-formed CPU tensors raise too
    with pytest.raises(RuntimeError, match="CUDA tensor"):
        te.tsdf_integrate(tsdf, weight, origin, 0.1, depth, ray, K, R, t, valid=valid)
    with pytest.raises(RuntimeError, match="CUDA tensor"):
        te.tsdf_surface_points(tsdf, weight, origin, 0.1, return_normals=True)
    with pytest.raises(RuntimeError, match="CUDA tensor"):
        te.tsdf_raycast(tsdf, weight, origin, 0.1, ray, R, t, 4, 5, 0.5, 0.05, 8)
    # dtype and type
    for args in ((tsdf.double(), weight, origin), (tsdf, weight.half(), origin), (tsdf, weight, origin.double()),
                 (tsdf.numpy(), weight, origin)):
        with pytest.raises(RuntimeError):
            te.tsdf_surface_points(*args, 0.1)


# ---------------------------------------------------------------------------------------------------------------------
# 4. the restatement against the truth of the plane, clean and noisy scenes
# ---------------------------------------------------------------------------------------------------------------------
def fused_scene(kind, seed, masked=True, **kw):
    """B=1, V=4, 48 x 64 into 48^3 over 1.6 m, trunc = 4 voxels -> dict: the scene, the grid, the volume, its points"""
    Bb, Vv, Hh, Ww = PLANE_SHAPE
    n, size, centre = PLANE_GRID
    sc = dict(fr.make_scene(kind, Bb, Vv, Hh, Ww, seed))
    sc["origin"], sc["voxel"] = tr.centred_grid(Bb, n, size, centre)
    sc["mask"] = sc["valid"]
    if masked:
        sc["mask"] = fr.consistency(sc["depth"], sc["ray"], sc["K"], sc["R"], sc["t"], sc["valid"], max_rel=0.01, min_views=1)[1]
    sc["tsdf"], sc["weight"] = tr.integrate(*tr.volume(Bb, n, n, n), sc["origin"], sc["voxel"], sc["depth"], sc["ray"], sc["K"],
                                            sc["R"], sc["t"], sc["mask"], **kw)
    sc["points"], sc["normals"], sc["src"], sc["n_per_track"] = tr.surface_points(sc["tsdf"], sc["weight"], sc["origin"],
                                                                                 sc["voxel"])
    return sc


@pytest.fixture(scope="module")
def plane():
    return fused_scene("plane", PLANE_SEED)


@pytest.fixture(scope="module")
def plane_all():
    """the plane with every pixel integrated (valid of the scene, all ones): what a view sees is then geometry alone"""
    return fused_scene("plane", PLANE_SEED, masked=False)


def test_integrate_measures_the_distance_along_the_view(plane_all):
    """On "plane", tsdf * trunc of a voxel is the mean, over the views that see it, of the true signed distance of the
    voxel from the plane along the view's z axis, clamped at trunc.

    The bound.  A view reads the surface depth at the pixel q nearest to the voxel's projection u, at most half a pixel
    away along each image axis.  In the view's frame the plane is n' . X = c and its depth along the ray through pixel
    (u, v) is z = c / (n' . r), r = ((u - cx) / f, (v - cy) / f, 1), so |dz/du| = z^2 |n'_x| / (f c) and |dz/dv| =
    z^2 |n'_y| / (f c).  Hence |z(q) - z(u)| <= 0.5 * (|n'_x| + |n'_y|) * z_max^2 / (f c) with z_max the largest depth of
    the view, taken 1 % larger for the variation of z over the half pixel; the f32 rounding of z (2^-24 * 2.8) is four
    orders below it.  The mean over the views is bounded by the largest of the views' bounds: 2.85e-3 here (measured:
    1.76e-3).  Voxels whose membership of a view hangs on the rounding are left out: those within one pixel of the
    image border and those whose distance is within the bound of -trunc."""
    sc = plane_all
    n = PLANE_GRID[0]
    Vv, Hh, Ww = PLANE_SHAPE[1:]
    voxel = np.float64(sc["voxel"])
    trunc = 4 * voxel
    X = np.stack(tr.centres(sc["origin"][0], sc["voxel"], n, n, n), 1).astype(np.float64)
    K = sc["K"].astype(np.float64)
    f, (nw, c) = K[0, 0], fr.PLANE
    bounds, seen, dist, sure = [], [], [], np.ones(len(X), bool)
    for v in range(Vv):
        Rm, tv = sc["R"][0, v].astype(np.float64), sc["t"][0, v].astype(np.float64)
        S = X @ Rm.T + tv
        n_cam, c_cam = Rm @ nw, c + (Rm @ nw) @ tv                 # n . X = c  <=>  (R n) . S = c + (R n) . t
        z_true = c_cam / (S @ n_cam / S[:, 2])
        d = z_true - S[:, 2]
        u, w = f * S[:, 0] / S[:, 2] + K[0, 2], f * S[:, 1] / S[:, 2] + K[1, 2]
        bound = 0.5 * (abs(n_cam[0]) + abs(n_cam[1])) * (1.01 * float(sc["depth"][0, v].max())) ** 2 / (f * c_cam)
        inside = (S[:, 2] > 0) & (u > 0.5) & (u < Ww - 1.5) & (w > 0.5) & (w < Hh - 1.5)
        outside = (S[:, 2] <= 0) | (u < -1.5) | (u > Ww + 0.5) | (w < -1.5) | (w > Hh + 0.5)
        sure &= (inside & (np.abs(d + trunc) > bound)) | outside
        seen.append(inside & (d > -trunc))
        dist.append(np.minimum(d, trunc))
        bounds.append(bound)
    seen, dist = np.array(seen), np.array(dist)
    count = seen.sum(0)
    T, w = sc["tsdf"].reshape(-1).astype(np.float64), sc["weight"].reshape(-1)
    assert sure.mean() > 0.8 and (count[sure] > 0).mean() > 0.3 and (count[sure] == 0).any()
    assert np.array_equal(w[sure], count[sure].astype(F))          # the weight is the number of views that see the voxel
    m = sure & (count > 0)
    want = (seen * dist).sum(0)[m] / count[m]
    err = np.abs(T[m] * trunc - want)
    print("integrate on the plane: largest |tsdf * trunc - mean distance| %.3e over %d voxels, bound %.3e; %.1f %% of the "
          "voxels compared, %.1f %% of those seen by no view" % (err.max(), m.sum(), max(bounds), 100 * sure.mean(),
                                                                100 * (count[sure] == 0).mean()))
    assert err.max() <= max(bounds)
    use = tr.usable_mask(sc["tsdf"], sc["weight"]).reshape(-1)
    assert (use & m).sum() > 5000                                  # the band around the plane is in it
    # a voxel that no view saw keeps the 1 it was made with
    assert (sc["tsdf"].reshape(-1)[w == 0] == 1).all() and (w == 0).any()
    # the grid reaches outside every frustum
    assert (count[sure] == 0).mean() > 0.05


def test_the_weights_stop_at_max_weight(plane_all):
    plane = plane_all
    capped = fused_scene("plane", PLANE_SEED, masked=False, max_weight=2.0)
    assert plane["weight"].max() == 4 and set(np.unique(plane["weight"])) == {0, 1, 2, 3, 4}
    assert np.array_equal(capped["weight"], np.minimum(plane["weight"], F(2)))
    early = plane["weight"] <= 2                                   # up to the second observation nothing differs
    assert np.array_equal(capped["tsdf"][early], plane["tsdf"][early])
    assert not np.array_equal(capped["tsdf"], plane["tsdf"])        # behind it the later views count for more


def test_surface_points_of_the_plane(plane):
    """largest distance to the plane 1.60e-3 (bound 2.0e-3); largest angle of a normal to the plane's 2.15 degrees
    (pinned at 4.30)"""
    sc = plane
    pts, nrm, src = sc["points"], sc["normals"], sc["src"]
    assert len(pts) > 2000 and sc["n_per_track"].tolist() == [len(pts)] and (np.diff(src) > 0).all()
    d = tr.plane_distance(pts, fr.PLANE)
    has = np.isfinite(nrm).all(1)
    assert np.array_equal(has, ~np.isnan(nrm).any(1)) and has.mean() > 0.9
    n_true = -fr.PLANE[0] / np.linalg.norm(fr.PLANE[0])            # towards free space: towards the cameras
    n64 = nrm[has].astype(np.float64)
    ang = np.rad2deg(np.arctan2(np.linalg.norm(np.cross(n64, n_true), axis=1), n64 @ n_true))
    print("plane: %d points, largest distance %.3e; %d normals, largest angle %.3f degrees" % (len(pts), d.max(), has.sum(),
                                                                                           ang.max()))
    assert d.max() <= MAX_PLANE_DIST
    assert ang.max() <= MAX_PLANE_NORMAL_DEG
    assert np.abs(np.linalg.norm(n64, axis=1) - 1).max() < 3e-7


def test_surface_points_of_the_clean_scene():
    """the share of points farther than one voxel from both planes: 3.11 % measured, capped at 6.22 % (and at 10 %)"""
    sc = fused_scene("clean", PLANE_SEED)
    pts = sc["points"]
    far = (tr.plane_distance(pts, fr.PLANE) > sc["voxel"]) & (np.abs(pts[:, 2].astype(np.float64) - fr.PATCH[1]) > sc["voxel"])
    near_patch = np.abs(pts[:, 2].astype(np.float64) - fr.PATCH[1]) <= sc["voxel"]
    print("clean: %d points, %d on the patch, %.2f %% farther than a voxel from both planes" % (len(pts), near_patch.sum(),
                                                                                              100 * far.mean()))
    assert near_patch.sum() > 100                                   # both surfaces are there
    assert far.mean() <= min(MAX_CLEAN_FAR_SHARE, 0.10)


@pytest.mark.parametrize("seed", [5, 6])
def test_surface_points_of_the_noisy_scene_beat_the_kept_points(seed):
    """median distance to the true surfaces, surface points over kept per-view points: 0.592 / 0.585 (asserted <= 0.75);
    without the mask 4.65 / 4.53: the volume is then worse than the raw points"""
    ratios = {}
    for masked in (True, False):
        sc = fused_scene("noisy", seed, masked)
        d_model = np.median(tr.scene_surface_distance(sc["points"]))
        per_view = tr.view_points(sc["depth"], sc["ray"], sc["R"], sc["t"], fr.live_mask(sc["depth"], sc["mask"]))
        d_views = np.median(tr.scene_surface_distance(per_view))
        ratios[masked] = d_model / d_views
        print("noisy, seed %d, valid=%s: median distance %.3e (surface points) against %.3e (per-view points): %.3f" % (
            seed, "keep" if masked else "valid", d_model, d_views, ratios[masked]))
    assert ratios[True] <= MAX_NOISY_RATIO
    assert ratios[False] > 1.0                                      # what README's advice (valid=keep) rests on


# ---------------------------------------------------------------------------------------------------------------------
# 5. the ray cast and frame-to-model alignment on the corner scene
# ---------------------------------------------------------------------------------------------------------------------
def corner_model(seed=CORNER_SEED):
    """tests/tsdf_ref.make_corner_model at the shape, grid and seed of this file"""
    return tr.make_corner_model(CORNER_SHAPE, seed, CORNER_DIMS, CORNER_VOXEL, CORNER_CENTRE)


def cast_statistics(sc, cast):
    """per cast pose: the share of the pixels whose true point lies inside the grid that hit, and the median
    |depth - truth| over the pixels that hit, in voxels"""
    Hh, Ww = CORNER_SHAPE[2:]
    out = []
    for v in range(cast.shape[1]):
        truth = sc["truth_cast"][0, v].astype(np.float64)
        P = truth.reshape(-1, 1) * sc["ray"].astype(np.float64) - sc["t_cast"][0, v].astype(np.float64)
        g = (P @ sc["R_cast"][0, v].astype(np.float64) - sc["origin"][0].astype(np.float64)) / sc["voxel"]
        inside = ((g >= 0) & (g <= np.asarray(CORNER_DIMS) - 1)).all(1).reshape(Hh, Ww)
        hit = np.isfinite(cast[0, v])
        err = np.abs(cast[0, v].astype(np.float64) - truth)[hit] / sc["voxel"]
        out.append(((hit & inside).sum() / inside.sum(), float(np.median(err)), float(err.max()), int(inside.sum())))
    return out


def model_track(sc, cast):
    """view 0 = the model seen from the pose of view 4, view 1 = the real view 1 with its pose off by 1 degree / 1 cm
    -> depth, R, t (the perturbed start), and the true R, t"""
    depth = np.ascontiguousarray(np.stack([cast[:, 1], sc["depth"][:, 1]], 1))
    R0 = np.ascontiguousarray(np.stack([sc["R"][:, 4], sc["R0"][:, 1]], 1))
    t0 = np.ascontiguousarray(np.stack([sc["t"][:, 4], sc["t0"][:, 1]], 1))
    return depth, R0, t0, np.stack([sc["R"][:, 4], sc["R"][:, 1]], 1), np.stack([sc["t"][:, 4], sc["t"][:, 1]], 1)


@pytest.fixture(scope="module")
def corner():
    sc = corner_model()
    vw = sc["views"]
    sc["tsdf"], sc["weight"] = tr.integrate(*tr.volume(1, *CORNER_DIMS), sc["origin"], sc["voxel"], vw["depth"], sc["ray"],
                                            sc["K"], vw["R"], vw["t"])
    sc["cast"] = tr.raycast(sc["tsdf"], sc["weight"], sc["origin"], sc["voxel"], sc["ray"], sc["R_cast"], sc["t_cast"],
                            *CORNER_SHAPE[2:], **CAST)
    # the chain as documented: only what the consistency check keeps goes into the volume
    kept = tr.integrate(*tr.volume(1, *CORNER_DIMS), sc["origin"], sc["voxel"], vw["depth"], sc["ray"], sc["K"], vw["R"], vw["t"],
                        vw["keep"])
    sc["cast_keep"] = tr.raycast(*kept, sc["origin"], sc["voxel"], sc["ray"], sc["R_cast"], sc["t_cast"], *CORNER_SHAPE[2:],
                                 **CAST)
    return sc


def test_the_ray_cast_finds_the_corner(corner):
    """at the pose of view 0 and of view 4 (not integrated): 97.6 % of the pixels whose true point lies inside the grid
    hit (>= 90 % asserted); median |depth - truth| 0.0107 / 0.0103 voxel, pinned at 0.0214 voxel"""
    stats = cast_statistics(corner, corner["cast"])
    for v, (share, med, worst, n_inside) in enumerate(stats):
        print("cast pose %d: %.2f %% of %d pixels hit, median error %.4f voxel, largest %.4f voxel" % (v, 100 * share, n_inside,
                                                                                                     med, worst))
        assert n_inside > 0.95 * CORNER_SHAPE[2] * CORNER_SHAPE[3]
        assert share >= MIN_HIT_SHARE
        assert med <= MAX_CAST_MEDIAN_VOXELS


def test_a_ray_that_starts_behind_the_wall_sees_nothing(corner):
    sc = corner
    behind = tr.raycast(sc["tsdf"], sc["weight"], sc["origin"], sc["voxel"], sc["ray"], sc["R_cast"], sc["t_cast"],
                        *CORNER_SHAPE[2:], d_min=2.7, step=0.048, n_steps=8)
    assert sc["truth_cast"].max() < 2.7 and np.isnan(behind).all()
    # some of them start inside the band behind the surface, where the first sample is defined and negative
    first = tr.raycast(sc["tsdf"], sc["weight"], sc["origin"], sc["voxel"], sc["ray"], sc["R_cast"], sc["t_cast"],
                       *CORNER_SHAPE[2:], d_min=2.7, step=0.048, n_steps=1)
    assert np.isnan(first).all()
    use = tr.usable_mask(sc["tsdf"], sc["weight"])
    assert (sc["tsdf"][use] < 0).any()


def test_frame_to_model_alignment(corner):
    """view 1 (1 degree / 1 cm off) against the model (valid = keep) cast at the pose of view 4, 6 rounds of the ICP
    restatement: translation error 9.70e-3 -> 3.26e-4, rotation error 1.000 -> 1.78e-2 degrees; pinned at 6.52e-4 and
    3.56e-2"""
    depth, R0, t0, R_true, t_true = model_track(corner, corner["cast_keep"])
    R, t, info = ir.depth_icp(depth, corner["ray"], corner["K"], R0, t0, None, iters=F2M_ITERS)
    rot0, tr0 = ir.pose_errors(R0, t0, R_true, t_true)
    rot1, tr1 = ir.pose_errors(R, t, R_true, t_true)
    print("frame to model: translation error %.3e -> %.3e, rotation error %.4f -> %.3e degrees, count %d" % (
        tr0[0, 1], tr1[0, 1], rot0[0, 1], rot1[0, 1], info["count"][-1, 0, 1]))
    assert info["ok"].tolist() == [[0, 1]] and np.array_equal(R[:, 0], R0[:, 0]) and np.array_equal(t[:, 0], t0[:, 0])
    assert abs(rot0[0, 1] - 1.0) < 1e-4 and abs(tr0[0, 1] - 0.01) < 1.5e-3
    assert tr1[0, 1] <= MAX_F2M_T_ERR and rot1[0, 1] <= MAX_F2M_ROT_ERR_DEG
