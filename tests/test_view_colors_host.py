"""CPU-only checks of the view colours (include/ctd_hip_mesh_color.h: ctd_mesh_view_colors_f32;
connecting_the_dots_amd.meshcolor): the rule's sentences (the header against its ctypes table: tests/test_abi_and_host.py),
argument validation before any HIP call, the Python module's own rejections and to_uint8 on CPU tensors, the restatement
tests/viewcolor_ref.py against hand-made answers and against the float64 ray caster of tests/chain_scene.py.

Restatement (numpy f32) against float64 truth on the chain scene: both tracks, V = 4 views of 64 x 256, 6000 area-weighted
surface samples per track, margin 0.01, no normals.  Per (point, view) the truth casts the unit ray from the camera
centre with chain_scene.ray_mesh: visible when the smallest positive hit parameter is >= len - margin + 0.001, occluded
when it is <= len - margin - 0.001, unsure in between.  Measured here:
  track 0: in-image pairs per view 842 .. 863, unsure 0 .. 0.12 %, visible 54.3 .. 67.0 %, occluded 33.0 .. 45.6 %
  track 1: in-image pairs per view 2367 .. 2707, unsure 0.33 .. 0.42 %, visible 39.1 .. 45.2 %, occluded 54.5 .. 60.5 %
(most samples of track 0 fall on the parts of its wall that no view has in its image).
Outside the unsure zone the restatement's UNOCCLUDED bit equals the truth without exception.

Colour truth: the views painted from the float64 cast with g_c(X) = 0.5 + 0.25 sin(2 X_c + c), C = 3.  For the points
all of whose used views sample their own surface (the 4 x 4 pixels around the float64 projection all hit it; 390 and 573
points), the largest |colour - g(X)| of the restatement over both tracks, both modes and the three channels is 8.72e-05
(track 0; 2.33e-05 on track 1; bilinear interpolation of a curved field under perspective, f32 rounding included);
COLOR_TOL is four times that."""
import functools
import os

import numpy as np
import pytest
import torch

from tests import chain_scene
from tests import viewcolor_ref as vr
from tests.test_tsdf_host import _Bufs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COLOR_HEADER = os.path.join(ROOT, "include", "ctd_hip_mesh_color.h")
OK, INVALID_ARG, UNSUPPORTED = 0, 1, 3
F = np.float32
NAN, INF = float("nan"), float("inf")
MARGIN = 0.01
COLOR_MEASURED = 8.72e-05
COLOR_TOL = 4 * COLOR_MEASURED


@pytest.fixture(scope="module")
def L():
    from connecting_the_dots_amd import _lib
    return _lib.lib()


# ---------------------------------------------------------------------------------------------------------------------
# 1. the header (header == ctypes table == exports: tests/test_abi_and_host.py, for every header)
# ---------------------------------------------------------------------------------------------------------------------
def test_the_header_states_the_rule():
    text = " ".join(open(COLOR_HEADER).read().replace("*", " ").split())
    for phrase in ("Everything is f32 and uncontracted, in the written association, with IEEE division and sqrtf",
                   "the views v = 0 .. V-1 are visited in ascending order",
                   "a step that fails ends the view",
                   "uvd2 > 0 is required",
                   "compared in f32, so a NaN fails",
                   "x0 = fminf(floorf(x), W-2) and fx = x - x0",
                   "all four pixels (y0 | y0+1, x0 | x0+1) of view v must be nonzero",
                   "Cv_c = -((R[0][c] t0 + R[1][c] t1) + R[2][c] t2)",
                   "cosv = dot(n, d) / sqrtf(dot(d, d))",
                   "cosv > 0 and cosv >= min_cos are required, so a NaN normal fails every view",
                   "With normals == NULL the step always passes and w = 1",
                   "dir = e / len (three divisions), t_max = len - margin",
                   "with ft > 0 and ft < t_max",
                   "Faces with an index outside [0, n_verts) are skipped and never dereferenced on the brute-force path",
                   "With n_faces == 0 nothing occludes",
                   "The answer is a boolean, so it is independent of the order in which the faces are visited",
                   "s_c = top + fy (bot - top)",
                   "A view with flags == 7 is used",
                   "acc_c = acc_c + w s_c and wsum = wsum + w over the used views in ascending v",
                   "color_c = acc_c / wsum and weight = wsum",
                   "the used view of largest w, the lowest v on a tie",
                   "With no used view color is NaN and weight is 0",
                   "The same bits on every run and on both paths",
                   "One lane owns one point: no atomics",
                   "this kernel is the definition",
                   "left at the first accepted hit",
                   "A non-finite origin, direction or t_max prunes nothing",
                   "CTD_ERR_UNSUPPORTED for a tree deeper than the traversal stack",
                   "There is no workspace",
                   "n_points == 0 is CTD_OK and touches nothing"):
        assert phrase in text, phrase


# ---------------------------------------------------------------------------------------------------------------------
# 2. validation before any HIP call
# ---------------------------------------------------------------------------------------------------------------------
NAMES = ["points", "normals", "images", "valid", "K", "R", "t", "verts", "faces", "bvh", "color", "weight", "n_views",
         "flags"]


def test_rejections_need_no_gpu(L):
    bufs = _Bufs(NAMES)                                               # 4 KiB apart: 10 points, 3 views of 1 x 4 x 5 fit

    def call(n=10, V=3, C=1, H=4, W=5, nv=10, nf=10, margin=0.01, min_cos=0.0, mode=0, **ptrs):
        p = dict(bufs.ptr, **ptrs)
        return L.ctd_mesh_view_colors_f32(p["points"], p["normals"], n, p["images"], p["valid"], p["K"], p["R"], p["t"],
                                          V, C, H, W, p["verts"], nv, p["faces"], nf, p["bvh"], margin, min_cos, mode,
                                          p["color"], p["weight"], p["n_views"], p["flags"], -1, None)

    invalid = [dict(n=-1), dict(nv=-1), dict(nf=-1), dict(V=0), dict(V=65), dict(C=0), dict(C=5), dict(H=1), dict(W=1),
               dict(mode=2), dict(mode=-1)]
    invalid += [dict(margin=m) for m in (-1e-3, NAN, INF, -INF)]
    invalid += [dict(min_cos=c) for c in (-0.1, 1.0, 2.0, NAN, INF)]
    invalid += [{k: None} for k in ("points", "images", "K", "R", "t", "color", "weight", "n_views", "faces", "verts")]
    invalid += [dict(bvh=bufs.ptr["bvh"] + 4), dict(bvh=bufs.ptr["bvh"] + 8), dict(n=0, nf=-1), dict(n=0, V=65),
                dict(n=0, bvh=bufs.ptr["bvh"] + 4), dict(n=0, margin=NAN)]
    for kw in invalid:
        assert call(**kw) == INVALID_ARG, kw
    unsupported = [dict(H=(1 << 24) + 1, W=2), dict(H=2, W=(1 << 24) + 1), dict(V=64, C=4, H=1 << 12, W=1 << 11),
                   dict(n=(1 << 31) // 3 + 1, V=1), dict(n=1 << 25, V=64), dict(nf=(1 << 28) + 1)]
    for kw in unsupported:
        assert call(**kw) == UNSUPPORTED, kw
    assert call(V=65, H=(1 << 24) + 1) == INVALID_ARG                 # the invalid class comes first
    # an output overlapping any other buffer of the call
    p = bufs.ptr
    for kw in (dict(color=p["points"]), dict(weight=p["images"] + 16), dict(n_views=p["R"]), dict(flags=p["t"]),
               dict(color=p["weight"]), dict(flags=p["color"] + 36), dict(n_views=p["weight"] + 36), dict(weight=p["K"] + 32),
               dict(color=p["verts"] + 100), dict(weight=p["faces"]), dict(flags=p["valid"] + 59), dict(color=p["normals"]),
               dict(n_views=p["bvh"] + 64)):
        assert call(**kw) == INVALID_ARG, kw
    assert call(H=(1 << 24) + 1, color=p["points"]) == UNSUPPORTED   # ... and the overlap check last
    # nothing to do: CTD_OK before any HIP call
    assert call(n=0) == OK and call(n=0, bvh=None, flags=None, normals=None, valid=None) == OK
    assert call(n=0, points=None, images=None, K=None, R=None, t=None, color=None, weight=None, n_views=None, nf=0,
                verts=None, faces=None) == OK


def _fake_bvh(verts, faces, usable=True):
    from connecting_the_dots_amd import renderer
    b = renderer.MeshBVH.__new__(renderer.MeshBVH)                   # the build needs a GPU; `matches` and `usable` do not
    b.verts, b.faces, b.usable = verts, faces, usable
    return b


PINNED = {
    "mesh": ["TsdfMesh", "load_ply", "save_ply", "tsdf_mesh"],
    "meshops": ["CleanMesh", "clean_tsdf_mesh", "mesh_clean", "mesh_components"],
    "mesheval": ["point_mesh_distance", "reconstruction_error", "sample_surface"],
}


def _own_names(mod):
    return sorted(n for n in vars(mod) if not n.startswith("_") and
                  getattr(getattr(mod, n), "__module__", "") == mod.__name__)


def test_meshcolor_imports_without_cuda_and_leaves_the_pinned_surfaces_alone():
    import importlib
    import subprocess
    import sys
    code = ("import torch, connecting_the_dots_amd.meshcolor as m; "
            "assert not torch.cuda.is_initialized(); print(m.USED)")
    out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip() == "7", out.stderr
    from connecting_the_dots_amd import meshcolor
    from connecting_the_dots_amd.torchext import functions
    assert _own_names(meshcolor) == ["ViewColors", "color_tsdf_mesh", "to_uint8", "view_colors"]
    assert (meshcolor.IN_IMAGE, meshcolor.FACING, meshcolor.UNOCCLUDED, meshcolor.USED) == (1, 2, 4, 7)
    assert len(functions.__all__) == 65 and not any("color" in n for n in functions.__all__)
    for name, want in PINNED.items():
        assert _own_names(importlib.import_module("connecting_the_dots_amd." + name)) == want, name
    t = meshcolor.AUTO_BVH_MIN_FACES
    assert t >= 2 and t & (t - 1) == 0                                # a power of two


def test_meshcolor_rejections_need_no_gpu():
    from connecting_the_dots_amd import _meshargs, mesh, meshcolor
    resolve = lambda *a: _meshargs._resolve_bvh(*a, meshcolor.AUTO_BVH_MIN_FACES)     # noqa: E731  as view_colors calls it
    p, im = torch.zeros(4, 3), torch.zeros(2, 3, 4, 5)
    K, R, t = torch.eye(3), torch.eye(3).repeat(2, 1, 1), torch.zeros(2, 3)
    with pytest.raises(RuntimeError, match="CUDA tensor"):
        meshcolor.view_colors(p, im, K, R, t, 0.01)
    with pytest.raises(RuntimeError, match="must be a tensor"):
        meshcolor.view_colors(p.numpy(), im, K, R, t, 0.01)
    with pytest.raises(TypeError):
        meshcolor.view_colors(p, im, K, R, t)                          # margin has no default
    with pytest.raises(RuntimeError, match="mesh.TsdfMesh"):
        meshcolor.color_tsdf_mesh((p, p), im[None], K, R[None], t[None], 0.01)
    import unittest.mock as mock
    with mock.patch.object(meshcolor, "_check", lambda *a, **k: None):   # the device check comes first: step over it
        views = lambda *a, **k: meshcolor._views(*a, who="view_colors", **k)     # noqa: E731
        assert views(im, K, R, t)[1:] == (2, 3, 4, 5)
        got = views(im[:, 0], K, R, t)                                 # [V,H,W]: one channel
        assert got[1:] == (2, 1, 4, 5) and tuple(got[0].shape) == (2, 1, 4, 5)
        assert views(im[None], K, R[None], t[None], lead=(1,))[1:] == (2, 3, 4, 5)
        for bad, msg in ((dict(images=im[0, 0]), "images must be shaped"), (dict(images=im[None, None]), "images must be shaped"),
                         (dict(images=torch.zeros(65, 1, 4, 5), R=torch.zeros(65, 3, 3), t=torch.zeros(65, 3)),
                          "between 1 and 64 views"),
                         (dict(images=torch.zeros(2, 5, 4, 5)), "between 1 and 4 channels"),
                         (dict(images=torch.zeros(2, 3, 1, 5)), "at least 2 x 2"),
                         (dict(K=torch.eye(4)), r"K must be shaped \[3,3\]"),
                         (dict(R=R[:1]), "R must be shaped"), (dict(t=t[:, :2]), "R must be shaped"),
                         (dict(R=R.reshape(2, 9)), "R must be shaped")):
            with pytest.raises(RuntimeError, match=msg):
                views(**dict(dict(images=im, K=K, R=R, t=t), **bad))
        with pytest.raises(RuntimeError, match="images must be shaped"):
            views(im[None], K, R[None], t[None], lead=(2,))
    sc = lambda **k: meshcolor._scalars(**dict(dict(margin=0.01, min_cos=0.0, mode="mean", return_flags=False,    # noqa: E731
                                                    who="view_colors"), **k))
    assert sc() == (0.01, 0.0, 0) and sc(mode="best", min_cos=0.5, margin=0) == (0.0, 0.5, 1)
    for bad in (dict(margin=-1.0), dict(margin=NAN), dict(margin=INF), dict(margin="1"), dict(margin=True), dict(min_cos=-0.1),
                dict(min_cos=1.0), dict(min_cos=NAN), dict(mode="median"), dict(mode=0), dict(return_flags=1)):
        with pytest.raises(RuntimeError):
            sc(**bad)
    # the tree: of other tensors, unusable, of a wrong kind, 'auto' below the threshold
    v, f = torch.zeros(5, 3), torch.zeros(2, 3, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="other verts / faces"):
        resolve(_fake_bvh(v.clone(), f), v, f, "view_colors")
    for bad in ("bvh", 3, (v, f)):
        with pytest.raises(RuntimeError, match="None, 'auto' or a renderer.MeshBVH"):
            resolve(bad, v, f, "view_colors")
    good = _fake_bvh(v, f)
    assert resolve(good, v, f, "x") is good and resolve(None, v, f, "x") is None
    assert resolve(_fake_bvh(v, f, usable=False), v, f, "x") is None       # falls back to brute force
    assert resolve("auto", v, f, "x") is None                               # below the threshold: no build
    assert isinstance(mesh.TsdfMesh, type)


def test_to_uint8_on_cpu_tensors():
    from connecting_the_dots_amd import meshcolor
    c = torch.tensor([[0.0, 0.5, 1.0], [-1.0, 2.0, 0.25], [NAN, 0.5, 0.5], [0.1, INF, -INF], [1.0 / 255, 0.999, 0.002]])
    got = meshcolor.to_uint8(c)
    assert got.dtype == torch.uint8 and got.is_contiguous()
    assert got.tolist() == [[0, 128, 255], [0, 255, 64], [0, 0, 0], [26, 255, 0], [1, 255, 1]]
    assert meshcolor.to_uint8(c, fill=(255, 0, 7))[2].tolist() == [255, 0, 7]
    one = meshcolor.to_uint8(torch.tensor([[0.5], [NAN], [1.5]]), fill=(1, 2, 3))
    assert one.tolist() == [[128, 128, 128], [1, 2, 3], [255, 255, 255]]
    assert meshcolor.to_uint8(torch.zeros(0, 3)).shape == (0, 3)
    for bad in (dict(color=c.double()), dict(color=c[:, :2]), dict(color=c[0]), dict(color=c.numpy()), dict(fill=(0, 0)),
                dict(fill=(0, 0, 256)), dict(fill=(0.5, 0, 0)), dict(fill=(-1, 0, 0))):
        with pytest.raises(RuntimeError):
            meshcolor.to_uint8(**dict(dict(color=c), **bad))


# ---------------------------------------------------------------------------------------------------------------------
# 3. the restatement against hand-made answers
# ---------------------------------------------------------------------------------------------------------------------
def _ramp_views(V, C, H, W):
    """images[v][c][y][x] = 1000 v + 100 c + 10 y + x in small integers' eighths: every interpolation below is exact"""
    v, c, y, x = np.meshgrid(np.arange(V), np.arange(C), np.arange(H), np.arange(W), indexing="ij")
    return (v * 64 + c * 16 + y * 2 + x * 0.125).astype(F)


def test_restatement_on_a_hand_made_scene():
    H, W = 4, 8
    K = np.array([[4, 0, 3.5], [0, 4, 1.5], [0, 0, 1]], F)             # pixel = 4 X / Z + centre
    R = np.stack([np.eye(3), np.eye(3)]).astype(F)
    t = np.array([[0, 0, 0], [-0.5, 0, 0]], F)                         # the second camera sits at x = +0.5
    im = _ramp_views(2, 2, H, W)
    # a wall at z = 2 over x in [-4, 0]: it hides what lies behind it and to the left
    verts = np.array([[-4, -4, 2], [0, -4, 2], [0, 4, 2], [-4, 4, 2]], F)
    faces = np.array([[0, 1, 2], [0, 2, 3]])
    pts = np.array([[0.5, 0.25, 4],      # right of the wall for view 0 (x = 4, y = 1.75); view 1 sees it at x = 3.5
                    [-1.0, 0.0, 4],      # behind the wall for both
                    [-1.0, 0.0, 2],      # on the wall: len - margin ends just in front of it
                    [0.0, 0.0, -1],      # behind the cameras
                    [4.5, 0.0, 4],       # x = 8 > W - 1 in view 0; x = 7.5 in view 1 is outside too
                    [3.5, 1.5, 4]], F)   # x = 7 = W - 1 and y = 3 = H - 1 in view 0: the clamp, fx = fy = 1; x = 6.5 in view 1
    color, weight, n_views, flags = vr.view_colors(pts, im, K, R, t, 0.01, verts, faces)
    assert flags.tolist() == [[7, 7], [3, 3], [7, 7], [0, 0], [0, 0], [7, 7]]
    assert n_views.tolist() == [2, 0, 2, 0, 0, 2] and weight.tolist() == [2, 0, 2, 0, 0, 2]
    s0 = np.array([1.75 * 2 + 4 * 0.125, 16 + 1.75 * 2 + 4 * 0.125], F)
    s1 = s0 + F(64) - F(0.5 * 0.125)
    assert np.array_equal(color[0], (s0 + s1) / F(2))
    assert np.isnan(color[[1, 3, 4]]).all()
    best = vr.view_colors(pts, im, K, R, t, 0.01, verts, faces, mode=1)
    assert np.array_equal(best[0][5], np.array([3 * 2 + 7 * 0.125, 16 + 3 * 2 + 7 * 0.125], F))   # the tie: view 0
    assert np.array_equal(best[0][0], s0) and best[1].tolist() == [1, 0, 1, 0, 0, 1] and best[2].tolist() == n_views.tolist()
    # a margin larger than the distance: nothing can occlude; a face with an index out of range takes no part
    assert vr.view_colors(pts, im, K, R, t, 10.0, verts, faces)[3][1].tolist() == [7, 7]
    assert vr.view_colors(pts, im, K, R, t, 0.01, verts, np.array([[0, 1, 9], [0, -1, 3]]))[3][1].tolist() == [7, 7]
    assert vr.view_colors(pts, im, K, R, t, 0.01)[3][1].tolist() == [7, 7]
    # normals: the weight is the cosine; a normal facing away, a perpendicular one and a NaN one fail FACING
    nrm = np.array([[0, 0, -1], [0, 0, -1], [0, 0, 1], [0, 0, -1], [0, 0, -1], [np.nan, 0, 0]], F)
    color, weight, n_views, flags = vr.view_colors(pts, im, K, R, t, 0.01, verts, faces, normals=nrm)
    assert flags.tolist() == [[7, 7], [3, 3], [1, 1], [0, 0], [0, 0], [1, 1]]
    c0 = F(4) / np.sqrt(F(0.5 * 0.5 + 0.25 * 0.25) + F(16))
    assert weight[0] == c0 + F(4) / np.sqrt(F(0.25 * 0.25) + F(16)) and 1.9 < weight[0] < 2
    perp = np.array([[0, 1, 0]], F)
    assert vr.view_colors(pts[2:3] * [1, 0, 1], im, K, R, t, 0.01, normals=perp)[3].tolist() == [[1, 1]]
    assert vr.view_colors(pts[:1], im, K, R, t, 0.01, normals=nrm[:1], min_cos=0.9999)[3].tolist() == [[1, 1]]
    # valid: one of the four pixels of view 0 is masked out
    valid = np.ones((2, H, W), np.uint8)
    valid[0, 2, 5] = 0
    got = vr.view_colors(pts[:1], im, K, R, t, 0.01, verts, faces, valid=valid)
    assert got[3].tolist() == [[0, 7]] and np.array_equal(got[0][0], s1)


def test_ray_tri_restatement_accepts_and_rejects_like_the_c_code():
    tri = [np.array([[[0, 0, 1]]], F), np.array([[[1, 0, 1]]], F), np.array([[[0, 1, 1]]], F)]
    o = np.zeros((1, 1, 3), F)
    d = np.array([[0.25, 0.25, 1], [2, 2, 1], [-0.25, -0.25, -1], [1, 0, 0], [np.nan, 0, 1], [0, 0, 1], [1, 0, 1]], F)[:, None, :]
    acc, ft = vr.ray_tri(o, d, *tri)
    assert acc[:, 0].tolist() == [True, False, True, False, True, True, True]   # a NaN passes every rejection
    assert ft[0, 0] == 1 and ft[2, 0] == -1 and np.isnan(ft[4, 0]) and ft[5, 0] == 1 and ft[6, 0] == 1


# ---------------------------------------------------------------------------------------------------------------------
# 4. the restatement against the float64 ray caster
# ---------------------------------------------------------------------------------------------------------------------
N_SAMPLES = 6000


def field(X):
    """g_c(X) = 0.5 + 0.25 sin(2 X_c + c), float64 [..., 3]"""
    return 0.5 + 0.25 * np.sin(2.0 * np.asarray(X, np.float64) + np.arange(3))


def surface_samples(verts, faces, n, seed):
    """n area-weighted samples of the mesh -> (points f32 [n,3], face [n])"""
    rs = np.random.RandomState(seed)
    V = np.asarray(verts, np.float64)
    a, b, c = (V[faces[:, k]] for k in range(3))
    area = np.linalg.norm(np.cross(b - a, c - a), axis=1)
    f = rs.choice(len(faces), size=n, p=area / area.sum())
    r = rs.uniform(size=(n, 2))
    s = np.sqrt(r[:, :1])
    pts = (1 - s) * a[f] + s * (1 - r[:, 1:]) * b[f] + s * r[:, 1:] * c[f]
    return pts.astype(F), f


@functools.lru_cache(maxsize=None)
def track(b):
    """the samples of track b, its painted views, the restatement's answers in both modes and the float64 truth"""
    sc = chain_scene.scene()
    m = sc.meshes[b]
    H, W, V = chain_scene.H, chain_scene.W, chain_scene.V
    pts, face = surface_samples(m["verts"], m["faces"], N_SAMPLES, 40 + b)
    images = np.zeros((V, 3, H, W), F)
    for v in range(V):
        T = sc.truth[b][v]
        images[v] = np.where(T["hit"][None], np.moveaxis(field(T["X"]), 2, 0), 0.0).astype(F)
    mean = vr.view_colors(pts, images, sc.K, sc.R[b], sc.t[b], MARGIN, m["verts"], m["faces"], mode=0)
    best = vr.view_colors(pts, images, sc.K, sc.R[b], sc.t[b], MARGIN, m["verts"], m["faces"], mode=1)
    X = pts.astype(np.float64)
    visible, unsure, own = (np.zeros((len(pts), V), bool) for _ in range(3))
    K = sc.K.astype(np.float64)
    for v in range(V):
        R, t = sc.R[b, v].astype(np.float64), sc.t[b, v].astype(np.float64)
        C = -R.T @ t
        e = X - C
        length = np.linalg.norm(e, axis=1)
        t64, _ = chain_scene.ray_mesh(C, e / length[:, None], m["verts"], m["faces"])
        visible[:, v] = t64 >= length - MARGIN + 0.001
        unsure[:, v] = ~visible[:, v] & ~(t64 <= length - MARGIN - 0.001)
        # the 4 x 4 pixels around the float64 projection all hit the point's own surface (the truth's notion: face // 2)
        S = X @ R.T + t
        with np.errstate(all="ignore"):
            x, y = K[0, 0] * S[:, 0] / S[:, 2] + K[0, 2], K[1, 1] * S[:, 1] / S[:, 2] + K[1, 2]
        ok = (S[:, 2] > 0) & (x >= 1) & (x <= W - 3) & (y >= 1) & (y <= H - 3)
        ix, iy = np.where(ok, np.floor(x), 1).astype(int), np.where(ok, np.floor(y), 1).astype(int)
        surf = np.where(sc.truth[b][v]["face"] >= 0, sc.truth[b][v]["face"] // 2, -1)
        for dy in range(-1, 3):
            for dx in range(-1, 3):
                ok &= surf[iy + dy, ix + dx] == face // 2
        own[:, v] = ok
    return dict(pts=pts, face=face, images=images, mean=mean, best=best, visible=visible, unsure=unsure, own=own)


@pytest.mark.parametrize("b", [0, 1])
def test_restatement_occlusion_against_float64(b):
    T = track(b)
    flags = T["mean"][3]
    assert np.array_equal(flags, T["best"][3])
    in_image = (flags & vr.IN_IMAGE) != 0
    assert ((flags & vr.FACING) != 0)[in_image].all()                  # no normals: the step always passes
    unocc = (flags & vr.UNOCCLUDED) != 0
    for v in range(chain_scene.V):
        m = in_image[:, v]
        sure = m & ~T["unsure"][:, v]
        n, vis, occ = m.sum(), (sure & T["visible"][:, v]).sum(), (sure & ~T["visible"][:, v]).sum()
        print("track %d view %d: %d in-image pairs, unsure %.2f %%, visible %.1f %%, occluded %.1f %%"
              % (b, v, n, 100.0 * (m & T["unsure"][:, v]).sum() / n, 100.0 * vis / n, 100.0 * occ / n))
        assert np.array_equal(unocc[sure, v], T["visible"][sure, v])   # outside the unsure zone: no exceptions
        assert (m & T["unsure"][:, v]).sum() < 0.01 * n                # a condition, not a measurement
        assert n >= 500 and vis >= 0.25 * n and occ >= 0.25 * n   # both classes are well populated


def test_restatement_colours_against_the_field():
    worst, n_checked = 0.0, 0
    for b in range(chain_scene.B):
        T = track(b)
        flags = T["mean"][3]
        used = flags == vr.USED
        sel = used.any(1) & (~used | T["own"]).all(1)                  # every used view samples the point's own surface
        n_checked += sel.sum()
        want = field(T["pts"][sel])
        for name in ("mean", "best"):
            color, weight, n_views, _ = T[name]
            assert (n_views[sel] >= 1).all() and np.isfinite(color[sel]).all()
            assert np.array_equal(n_views, used.sum(1)) and np.isnan(color[n_views == 0]).all()
            err = np.abs(color[sel].astype(np.float64) - want).max()
            print("track %d, %s: %d points, max |colour - g(X)| %.3e (tolerance %.3e)" % (b, name, sel.sum(), err, COLOR_TOL))
            worst = max(worst, err)
            assert err <= COLOR_TOL
        assert np.array_equal(T["mean"][1][sel], n_views[sel].astype(F))       # w = 1: the weight is the count
        assert (T["best"][1][sel] == 1).all()
    assert n_checked >= 500
    print("largest error %.3e" % worst)
