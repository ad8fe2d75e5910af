"""GPU checks of the view colours (ctd_mesh_view_colors_f32 of include/ctd_hip_mesh_color.h, csrc/mesh_color.hip;
connecting_the_dots_amd.meshcolor): the brute-force kernel bit for bit against the restatement tests/viewcolor_ref.py on
all four outputs, the BVH traversal bit for bit against the brute-force kernel on points built so that every outcome
occurs, the fallback from a tree that is too deep, and color_tsdf_mesh on a two-track sphere volume.

The tolerance of the sphere's colours.  The views are painted analytically from the true spheres with the field
g_c(X) = 0.5 + 0.25 sin(GRAD_K (X_c - centre_c) + c), whose gradient is at most 0.25 GRAD_K per unit.  A mesh vertex lies
off the true sphere by dr (measured in the test from the vertices and the sphere alone, a property of the mesh), so the
sphere point a view sees along the ray through the vertex is at most dr / cos <= dr / MIN_COS from it (the view's ray
meets the surface at an angle whose cosine is at least MIN_COS), and the field differs by at most 0.25 GRAD_K dr / MIN_COS.
The interpolation error is the host test's COLOR_TOL: its field changes 20 times faster per unit than this one and its
pixels are 0.013 units wide at the scene's distance against 0.19 here, so the second-order error, (pixel width * rate)^2,
is half the host test's here; the sphere's own curvature under the projection adds 0.25 GRAD_K h^2 / (8 r cos^2) <= 6e-05
for h = 0.19 and r = 6.5.  Tolerance: COLOR_TOL + 0.25 GRAD_K dr_max / MIN_COS."""
import functools

import numpy as np
import pytest
import torch

from tests import bvh_scenes
from tests import mesh_ref as mr
from tests import viewcolor_ref as vr
from tests.test_point_mesh_gpu import deep_mesh
from tests.test_view_colors_host import COLOR_TOL

pytestmark = pytest.mark.gpu

DEV = "cuda"
F = np.float32
OK, UNSUPPORTED = 0, 3
NAN, INF = float("nan"), float("inf")


def dev(a, dtype=None):
    a = np.ascontiguousarray(a if dtype is None else np.asarray(a, dtype))
    return torch.from_numpy(a).to(DEV)


def raw(sc, n=None, bvh=None, want_flags=True, tensors=None):
    """one call of the C entry point on the scene `sc` (its first n points) -> (status, color, weight, n_views, flags) as
    numpy; the outputs start as garbage the kernel has to overwrite.  `tensors` keeps the device copies between calls."""
    from connecting_the_dots_amd import _lib
    t = tensors if tensors is not None else scene_tensors(sc)
    n = sc["points"].shape[0] if n is None else n
    V, C, H, W = sc["images"].shape
    color = torch.full((n, C), -7.0, dtype=torch.float32, device=DEV)
    weight = torch.full((n,), -7.0, dtype=torch.float32, device=DEV)
    n_views = torch.full((n,), -7, dtype=torch.int32, device=DEV)
    flags = torch.full((n, V), 0xA5, dtype=torch.uint8, device=DEV) if want_flags else None
    ptr = lambda x: x.data_ptr() if x is not None and x.numel() else None     # noqa: E731
    st = _lib.lib().ctd_mesh_view_colors_f32(
        ptr(t["points"]), ptr(t["normals"]), n, ptr(t["images"]), ptr(t["valid"]), ptr(t["K"]), ptr(t["R"]), ptr(t["t"]),
        V, C, H, W, ptr(t["verts"]), t["verts"].shape[0], ptr(t["faces"]), t["faces"].shape[0],
        None if bvh is None else bvh.buffer.data_ptr(), sc["margin"], sc["min_cos"], sc["mode"], ptr(color), ptr(weight),
        ptr(n_views), ptr(flags), torch.cuda.current_device(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return (st, color.cpu().numpy(), weight.cpu().numpy(), n_views.cpu().numpy(),
            None if flags is None else flags.cpu().numpy())


def scene_tensors(sc):
    t = {k: dev(sc[k], F) for k in ("points", "images", "K", "R", "t")}
    t["verts"] = dev(np.asarray(sc["verts"], F).reshape(-1, 3))
    t["faces"] = dev(np.asarray(sc["faces"], np.int32).reshape(-1, 3))
    t["normals"] = None if sc["normals"] is None else dev(sc["normals"], F)
    t["valid"] = None if sc["valid"] is None else dev(sc["valid"], np.uint8)
    return t


def reference(sc):
    return vr.view_colors(sc["points"], sc["images"], sc["K"], sc["R"], sc["t"], sc["margin"], sc["verts"], sc["faces"],
                          normals=sc["normals"], valid=sc["valid"], min_cos=sc["min_cos"], mode=sc["mode"])


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    if a.dtype == np.float32:
        return bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())
    return bool(np.array_equal(a, b))


def assert_same(got, want, what):
    for name, g, w in zip(("color", "weight", "n_views", "flags"), got, want):
        if g is None and w is None:
            continue
        if not same_bits(g, w):
            g2, w2 = g.reshape(len(g), -1), w.reshape(len(w), -1)
            both_nan = (g2 != g2) & (w2 != w2) if g2.dtype == np.float32 else np.zeros(g2.shape, bool)
            bad = np.where(((g2 != w2) & ~both_nan).any(1))[0]
            raise AssertionError("%s: %s differs at %d of %d points, first %s: %s vs %s" % (
                what, name, len(bad), len(g), bad[:5], g[bad[:3]], w[bad[:3]]))


# ---------------------------------------------------------------------------------------------------------------------
# scenes
# ---------------------------------------------------------------------------------------------------------------------
def intrinsics(H, W):
    """a focal length that is a power of two and a principal point at the centre of the pixel grid: the hand-placed points
    below project to exactly 0 and exactly W - 1"""
    f = float(1 << int(np.ceil(np.log2(max(H, W)))))
    return np.array([[f, 0, (W - 1) / 2.0], [0, f, (H - 1) / 2.0], [0, 0, 1]], F)


def small_rotation(rs, angle):
    w = rs.normal(size=3)
    w *= rs.uniform(0, angle) / np.linalg.norm(w)
    th = np.linalg.norm(w)
    k = w / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx


def poses(V, rs):
    """view 0 is the identity at the origin, view 1 (when there is one) repeats it -- a tie for mode 1 --, the others sit
    within 0.3 of the origin and look along +z up to 0.15 rad off"""
    R, t = [np.eye(3)], [np.zeros(3)]
    for v in range(1, V):
        if v == 1:
            R.append(R[0]), t.append(t[0])
            continue
        Rv, C = small_rotation(rs, 0.15), rs.uniform(-0.3, 0.3, size=3)
        R.append(Rv), t.append(-Rv @ C)
    return np.stack(R).astype(F), np.stack(t).astype(F)


def brute_mesh(name, n_faces):
    if name == "icosphere":
        v, f = bvh_scenes.icosphere(2)
        v = v * 0.6 + [0.1, -0.05, 3.0]
    else:
        v, _, f = bvh_scenes.get_mesh_like(500, 3)
    v, f = np.asarray(v, F), np.array(f[:n_faces], np.int32)
    if n_faces > 100:                                       # indices outside [0, n_verts): skipped, never dereferenced
        f[5], f[77] = [0, 1, len(v)], [-1, 2, 3]
    return v, f


def hand_placed(K, H, W, margin):
    """points for view 0 (identity pose at the origin): x exactly 0 and exactly W - 1, y exactly 0 and H - 1, just outside
    each, behind the camera, at the camera centre, with NaN and infinite coordinates, closer than margin"""
    f, cx, cy = float(K[0, 0]), float(K[0, 2]), float(K[1, 2])
    Z = 2.0
    X0, X1, Y0, Y1 = -Z * cx / f, Z * cx / f, -Z * cy / f, Z * cy / f
    eps = 1 + 1e-5
    return np.array([[X0, 0, Z], [X1, 0, Z], [0, Y0, Z], [0, Y1, Z], [X1, Y1, Z], [X0, Y0, Z],
                     [X0 * eps, 0, Z], [X1 * eps, 0, Z], [0, Y0 * eps, Z], [0, Y1 * eps, Z],
                     [0, 0, -1], [0.1, 0.1, -3], [0, 0, 0], [NAN, 0, 2], [0, NAN, 2], [0, 0, NAN], [INF, 0, 2], [0, 0, INF],
                     [0, 0, margin / 2], [0, 0, 2], [0, 0, 1e30]], F)


N_BRUTE = 300


def brute_scene(name, n_faces, V, C, H, W, mode, normals, valid, margin=0.01, min_cos=0.0, seed=0):
    rs = np.random.RandomState(1000 + seed)
    verts, faces = brute_mesh(name, n_faces)
    K = intrinsics(H, W)
    R, t = poses(V, rs)
    hand = hand_placed(K, H, W, margin)
    centres = np.stack([vr.camera_centre(R[v], t[v]) for v in range(min(V, 4))])      # len == 0 for their own view
    objects = verts[6:] if name != "icosphere" else verts
    n_rest = N_BRUTE - len(hand) - len(centres)
    near = objects[rs.randint(0, len(objects), n_rest // 3)] + rs.normal(size=(n_rest // 3, 3)) * 1e-3
    m = n_rest - n_rest // 3
    v = rs.randint(0, V, m)                                                            # pixels of random views, cast back
    uv1 = np.stack([rs.uniform(0, W - 1, m), rs.uniform(0, H - 1, m), np.ones(m)], 1)
    cam = uv1 @ np.linalg.inv(K.astype(np.float64)).T * rs.uniform(0.5, 8, size=(m, 1))
    back = np.einsum("nji,nj->ni", R[v].astype(np.float64), cam - t[v])
    points = np.concatenate([hand, centres, near, back]).astype(F)
    assert len(points) == N_BRUTE
    nrm = None
    if normals:
        nrm = -points.astype(np.float64) + rs.normal(size=points.shape) * 1.5           # roughly towards the cameras
        nrm[np.isnan(nrm) | np.isinf(nrm)] = 0.3
        nrm[19] = [1, 0, 0]                                    # perpendicular to view 0's line of sight to (0, 0, 2)
        nrm[0] = [NAN, 0, -1]
        nrm = nrm.astype(F)
    mask = None
    if valid:
        mask = rs.choice(np.array([0, 1, 255], np.uint8), size=(V, H, W), p=[0.12, 0.5, 0.38])
    images = rs.uniform(0, 1, size=(V, C, H, W)).astype(F)
    return dict(points=points, normals=nrm, images=images, valid=mask, K=K, R=R, t=t, verts=verts, faces=faces,
                margin=margin, min_cos=min_cos, mode=mode)


# name, n_faces, V, C, H, W, mode, normals, valid, min_cos
BRUTE_CASES = [
    ("icosphere", 320, 4, 3, 64, 256, 0, True, True, 0.0),
    ("icosphere", 0, 1, 1, 2, 2, 0, False, False, 0.0),
    ("icosphere", 255, 4, 4, 5, 7, 1, True, False, 0.0),
    ("icosphere", 256, 4, 1, 5, 7, 0, False, True, 0.0),
    ("icosphere", 257, 64, 3, 5, 7, 1, True, True, 0.25),
    ("like", 340, 4, 3, 64, 256, 1, False, False, 0.0),
    ("like", 340, 64, 4, 64, 256, 0, True, False, 0.3),
    ("like", 257, 1, 3, 2, 2, 0, True, False, 0.0),
]


# ---------------------------------------------------------------------------------------------------------------------
# 1. the brute-force kernel is the restatement, bit for bit
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", BRUTE_CASES, ids=lambda c: "%s-%df-V%d-C%d-%dx%d-m%d%s%s" % (
    c[:7] + ("-normals" if c[7] else "", "-valid" if c[8] else "")))
def test_brute_force_is_the_restatement(case):
    name, n_faces, V, C, H, W, mode, normals, valid, min_cos = case
    sc = brute_scene(name, n_faces, V, C, H, W, mode, normals, valid, min_cos=min_cos, seed=BRUTE_CASES.index(case))
    want = reference(sc)                                                       # once, for the 300 points
    flags = want[3]
    # the scene does what it was built for (the restatement alone says so)
    if not valid:
        assert (flags[:6, 0] & 1).all()                                        # exactly on the border: inside
    assert (flags[6:13, 0] == 0).all() and (flags[13:18] == 0).all()           # just outside, behind, the centre, non-finite
    if not valid and not normals:
        assert flags[18, 0] == 7                                               # len < margin: nothing occludes
    if normals:
        assert flags[19, 0] in (0, 1) and (flags[0] <= 1).all()                # the perpendicular and the NaN normal
    if n_faces >= 255 and H > 2:
        used, occ = (flags == 7).sum(), (flags == 3).sum()
        assert used > 20 and occ > 20, (used, occ)                             # both outcomes of the occlusion query
    if V >= 2 and not normals and not valid:
        assert (flags[:, 0] == flags[:, 1]).all()                              # the repeated pose: a tie for mode 1
    tensors = scene_tensors(sc)
    for n in (1, 63, 65, 257, 300):
        st, *got = raw(sc, n, tensors=tensors)
        assert st == OK
        assert_same(got, [w[:n] for w in want], "%s, %d points" % (case, n))
    st, *got = raw(sc, want_flags=False, tensors=tensors)                      # flags are optional
    assert st == OK and got[3] is None
    assert_same(got[:3], want[:3], "%s without flags" % (case,))
    if n_faces == 0:
        assert not (flags == 3).any()                                          # nothing occludes


def test_mode_1_takes_the_lower_view_on_a_tie_and_the_larger_cosine_otherwise():
    sc = brute_scene("icosphere", 320, 4, 3, 64, 256, 1, True, False, seed=50)
    st, color, weight, n_views, flags = raw(sc)
    want = reference(sc)
    assert st == OK
    assert_same((color, weight, n_views, flags), want, "mode 1")
    tie = (flags[:, 0] == 7) & (flags[:, 1] == 7)
    assert tie.sum() > 20
    # views 0 and 1 have one pose and different images: where no other view is used the colour must be view 0's sample
    only = tie & (flags[:, 2] != 7) & (flags[:, 3] != 7)
    one = dict(sc, R=sc["R"][:1], t=sc["t"][:1], images=sc["images"][:1])
    first = reference(one)
    assert only.sum() > 5 and same_bits(color[only], first[0][only]) and same_bits(weight[only], first[1][only])
    other = (flags == 7).sum(1) >= 3
    assert other.sum() > 5 and (weight[other] >= first[1][other]).all()


# ---------------------------------------------------------------------------------------------------------------------
# 2. the traversal is the brute-force kernel, bit for bit
# ---------------------------------------------------------------------------------------------------------------------
N_BVH = 4096


def bvh_mesh(name):
    if name == "icosphere":
        v, f = bvh_scenes.icosphere(3)
        return (v * 0.7 + [0, 0, 3]).astype(F), f.astype(np.int32), 0
    if name == "torus":
        v, f = bvh_scenes.torus(48, 40)
        return (v @ bvh_scenes.rand_rot(np.random.RandomState(3)).T + [0.2, 0, 3]).astype(F), f.astype(np.int32), 0
    v, _, f = bvh_scenes.get_mesh_like(5000, int(name))
    return v, f, 6                                            # the board's six corners come first


def bvh_scene(name, margin, seed):
    rs = np.random.RandomState(seed)
    verts, faces, first = bvh_mesh(name)
    H, W, V, C = 48, 64, 4, 3
    K = intrinsics(H, W)
    R, t = poses(V, rs)
    obj = faces[(faces >= first).all(1)]
    pick = obj[rs.randint(0, len(obj), N_BVH)]
    bary = rs.dirichlet([1, 1, 1], N_BVH)
    V64 = verts.astype(np.float64)
    on = (bary[:, :, None] * V64[pick]).sum(1)                                        # on the surface
    C0 = np.zeros(3)
    q = N_BVH // 8
    pts = on.copy()
    away = (on - C0) / np.linalg.norm(on - C0, axis=1, keepdims=True)
    pts[q:2 * q] += away[q:2 * q] * rs.uniform(0, 0.02, size=(q, 1))                  # margin-close behind it
    pts[2 * q:3 * q] += away[2 * q:3 * q] * rs.uniform(0.02, 0.3, size=(q, 1))        # inside or behind the objects
    pts[3 * q:4 * q] -= away[3 * q:4 * q] * rs.uniform(0, 0.5, size=(q, 1))           # in front of them
    pts[4 * q:5 * q] = C0 + away[4 * q:5 * q] * 1e3                                   # far away, behind an object
    pts[5 * q:6 * q] = C0 + away[5 * q:6 * q] * 1e10                                  # farther than the largest margin
    pts[6 * q:7 * q] = rs.uniform(-2, 2, size=(q, 3)) + [0, 0, 3]                     # anywhere
    weird = np.array([[NAN, 0, 2], [0, INF, 2], [-INF, NAN, 0], [1e30, 0, 1e30], [3e38, 3e38, 3e38], [0, 0, 0]], F)
    extra = np.concatenate([weird, np.stack([vr.camera_centre(R[v], t[v]) for v in range(V)]),
                            verts[rs.randint(first, len(verts), 27)]])
    points = np.concatenate([pts.astype(F), extra.astype(F)])
    assert len(points) == N_BVH + 37
    nrm = (-points.astype(np.float64) + rs.normal(size=points.shape)).astype(F)
    nrm[~np.isfinite(nrm)] = 0.5
    images = rs.uniform(0, 1, size=(V, C, H, W)).astype(F)
    return dict(points=points, normals=nrm if seed % 2 else None, images=images, valid=None, K=K, R=R, t=t, verts=verts,
                faces=faces, margin=margin, min_cos=0.0, mode=seed % 2)


@pytest.mark.parametrize("margin", [0.0, 0.01, 1e9])
@pytest.mark.parametrize("name", ["icosphere", "torus", "7"])
def test_bvh_is_brute_force(name, margin):
    from connecting_the_dots_amd import renderer
    sc = bvh_scene(name, margin, seed=len(name) + int(margin > 0) + int(margin > 1))
    tensors = scene_tensors(sc)
    bvh = renderer.MeshBVH(tensors["verts"], tensors["faces"])
    assert bvh.usable
    st, *ref = raw(sc, tensors=tensors)
    assert st == OK
    st, *got = raw(sc, bvh=bvh, tensors=tensors)
    assert st == OK
    assert_same(got, ref, "%s, margin %g" % (name, margin))
    flags = ref[3]
    visible, occluded = (flags == 7).sum(), (flags == 3).sum()
    print("%s, margin %g: %d visible and %d occluded pairs of %d" % (name, margin, visible, occluded, flags.size))
    assert visible > 100 and occluded > 100                                   # both outcomes, in every run
    st, *again = raw(sc, bvh=bvh, tensors=tensors)                            # the same bits on every run
    assert st == OK
    assert_same(again, got, "second call")


def test_a_tree_that_is_too_deep_falls_back_with_the_same_bits():
    from connecting_the_dots_amd import meshcolor, renderer
    verts, faces = deep_mesh()
    rs = np.random.RandomState(8)
    H, W, V = 48, 64, 4
    R, t = poses(V, rs)
    pts = np.concatenate([verts[::5] + rs.normal(size=verts[::5].shape) * 1e-4,
                          verts[::7] * [1, 1, 2], rs.uniform(-1, 1, size=(200, 3)) + [0, 0, 1]]).astype(F)
    sc = dict(points=pts, normals=None, images=rs.uniform(0, 1, size=(V, 3, H, W)).astype(F), valid=None, K=intrinsics(H, W),
              R=R, t=t, verts=verts.astype(F), faces=faces.astype(np.int32), margin=1e-3, min_cos=0.0, mode=0)
    tensors = scene_tensors(sc)
    bvh = renderer.MeshBVH(tensors["verts"], tensors["faces"])
    assert bvh.usable == (bvh.depth <= 62)
    st, *ref = raw(sc, tensors=tensors)
    assert st == OK and (ref[3] == 7).any()
    st, *got = raw(sc, bvh=bvh, tensors=tensors)
    assert st == (OK if bvh.usable else UNSUPPORTED)
    if bvh.usable:
        assert_same(got, ref, "deep tree")
    vc = meshcolor.view_colors(tensors["points"], tensors["images"], tensors["K"], tensors["R"], tensors["t"], 1e-3,
                               tensors["verts"], tensors["faces"], bvh=bvh, return_flags=True)     # usable or not
    assert_same([x.cpu().numpy() for x in (vc.color, vc.weight, vc.n_views, vc.flags)], ref, "view_colors with the deep tree")


# ---------------------------------------------------------------------------------------------------------------------
# 3. the Python module
# ---------------------------------------------------------------------------------------------------------------------
def test_view_colors_auto_none_and_an_explicit_tree_agree(monkeypatch):
    from connecting_the_dots_amd import meshcolor, renderer
    sc = bvh_scene("icosphere", 0.01, seed=3)
    want = reference(dict(sc, points=sc["points"][:500], normals=sc["normals"][:500]))
    T = scene_tensors(sc)
    args = (T["points"], T["images"], T["K"], T["R"], T["t"], 0.01, T["verts"], T["faces"])
    kw = dict(normals=T["normals"], mode="best", return_flags=True)
    built = []
    real = renderer.MeshBVH
    outs = [meshcolor.view_colors(*args, **kw), meshcolor.view_colors(*args, bvh=real(T["verts"], T["faces"]), **kw)]
    monkeypatch.setattr(renderer, "MeshBVH", lambda *a, **k: built.append(1) or real(*a, **k))      # counts 'auto' builds
    outs.append(meshcolor.view_colors(*args, bvh="auto", **kw))
    assert len(built) == (len(sc["faces"]) >= meshcolor.AUTO_BVH_MIN_FACES)
    monkeypatch.setattr(meshcolor, "AUTO_BVH_MIN_FACES", 1024)
    outs.append(meshcolor.view_colors(*args, bvh="auto", **kw))                                    # above it: builds
    assert len(built) >= 1
    monkeypatch.undo()
    for vc in outs:
        assert vc.color.dtype == torch.float32 and vc.n_views.dtype == torch.int32 and vc.flags.dtype == torch.uint8
        assert_same([x.cpu().numpy()[:500] for x in (vc.color, vc.weight, vc.n_views, vc.flags)], want, "view_colors")
        assert_same([x.cpu().numpy() for x in (vc.color, vc.weight, vc.n_views, vc.flags)],
                    [x.cpu().numpy() for x in (outs[0].color, outs[0].weight, outs[0].n_views, outs[0].flags)], "paths")
    assert meshcolor.view_colors(*args).flags is None
    one = meshcolor.view_colors(T["points"], T["images"][:, 0].contiguous(), T["K"], T["R"], T["t"], 0.01)   # [V,H,W], no mesh
    assert one.color.shape == (len(sc["points"]), 1) and not bool(((one.n_views > 0) & torch.isnan(one.color[:, 0])).any())
    bad = T["faces"].clone()
    bad[7, 1] = len(sc["verts"])                                     # 'auto' must not hand such faces to the tree's build
    monkeypatch.setattr(meshcolor, "AUTO_BVH_MIN_FACES", 1024)
    got = meshcolor.view_colors(T["points"][:500].contiguous(), *args[1:7], bad, bvh="auto", return_flags=True)
    monkeypatch.undo()
    want_bad = reference(dict(sc, points=sc["points"][:500], normals=None, faces=bad.cpu().numpy(), mode=0))
    assert_same([x.cpu().numpy() for x in (got.color, got.weight, got.n_views, got.flags)], want_bad, "a face out of range")
    with pytest.raises(RuntimeError, match="other verts / faces"):
        meshcolor.view_colors(*args, bvh=real(T["verts"].clone(), T["faces"]))
    with pytest.raises(RuntimeError, match="unsupported dtype"):
        meshcolor.view_colors(T["points"].double(), *args[1:])
    with pytest.raises(RuntimeError, match="unsupported dtype"):
        meshcolor.view_colors(*args[:7], T["faces"].long())
    with pytest.raises(RuntimeError, match=r"shaped \[n,3\]"):
        meshcolor.view_colors(T["points"].reshape(-1), *args[1:])
    with pytest.raises(RuntimeError, match="contiguous"):
        meshcolor.view_colors(T["points"][:, [2, 1, 0]].t().contiguous().t(), *args[1:])
    with pytest.raises(RuntimeError, match="one row per point"):
        meshcolor.view_colors(*args, normals=T["normals"][:5].contiguous())
    with pytest.raises(RuntimeError, match="valid must be shaped"):
        meshcolor.view_colors(*args, valid=torch.ones((4, 48, 63), dtype=torch.uint8, device=DEV))
    with pytest.raises(RuntimeError, match="verts and faces go together"):
        meshcolor.view_colors(*args[:7])
    empty = meshcolor.view_colors(T["points"][:0], *args[1:], return_flags=True)
    assert [tuple(x.shape) for x in (empty.color, empty.weight, empty.n_views, empty.flags)] == [(0, 3), (0,), (0,), (0, 4)]


SPHERE_N, SPHERE_R = 24, (8.0, 6.5)
GRAD_K = 0.1
MIN_COS = 0.5
SPHERE_MARGIN = 0.5
SPHERE_HW, SPHERE_F, SPHERE_DIST = (96, 128), 256.0, 48.0


def sphere_field(X, centre):
    return 0.5 + 0.25 * np.sin(GRAD_K * (np.asarray(X, np.float64) - centre) + np.arange(3))


def look_at(C, target):
    z = (target - C) / np.linalg.norm(target - C)
    x = np.cross([0.0, 1.0, 0.0], z)
    x /= np.linalg.norm(x)
    return np.stack([x, np.cross(z, x), z])                             # rows: the camera's axes in the world


@functools.lru_cache(maxsize=None)
def sphere_tracks():
    """two tracks: the volume of a sphere each, and four views around it painted from the true sphere with the field"""
    H, W = SPHERE_HW
    K = np.array([[SPHERE_F, 0, (W - 1) / 2.0], [0, SPHERE_F, (H - 1) / 2.0], [0, 0, 1]], F)
    dirs = np.array([[0, 0, -1], [0.7, 0.1, -0.7], [-0.7, 0.2, -0.6], [0.1, 0.8, -0.6]])
    Ts, ws, cs, Rs, ts, ims = [], [], [], [], [], []
    v, u = np.divmod(np.arange(H * W), W)
    cam = np.stack([(u - K[0, 2]) / K[0, 0], (v - K[1, 2]) / K[1, 1], np.ones(H * W)], 1).astype(np.float64)
    for b, r in enumerate(SPHERE_R):
        T, w, centre = mr.sphere_volume(SPHERE_N, r)
        R = np.stack([look_at(centre + SPHERE_DIST * d / np.linalg.norm(d), centre) for d in dirs]).astype(F)
        Cs = [centre + SPHERE_DIST * d / np.linalg.norm(d) for d in dirs]
        t = np.stack([-(R[i].astype(np.float64) @ Cs[i]) for i in range(len(dirs))]).astype(F)
        im = np.zeros((len(dirs), 3, H, W), F)
        for i in range(len(dirs)):                                      # the f32 pose, cast to float64, as the kernel has it
            R64, t64 = R[i].astype(np.float64), t[i].astype(np.float64)
            C = -R64.T @ t64
            d = cam @ R64
            d /= np.linalg.norm(d, axis=1, keepdims=True)
            oc = C - centre
            bq = d @ oc
            disc = bq * bq - (oc @ oc - r * r)
            s = -bq - np.sqrt(np.maximum(disc, 0))
            X = C + s[:, None] * d
            im[i] = np.where((disc > 0)[None], sphere_field(X, centre).T, 0.0).reshape(3, H, W).astype(F)
        Ts.append(T[0]), ws.append(w[0]), cs.append(centre), Rs.append(R), ts.append(t), ims.append(im)
    return dict(T=np.stack(Ts), w=np.stack(ws), centres=cs, K=K, R=np.stack(Rs), t=np.stack(ts), images=np.stack(ims))


def test_color_tsdf_mesh(tmp_path, monkeypatch):
    from connecting_the_dots_amd import mesh, meshcolor, renderer
    S = sphere_tracks()
    B, V = len(SPHERE_R), S["R"].shape[1]
    H, W = SPHERE_HW
    m = mesh.tsdf_mesh(dev(S["T"]), dev(S["w"]), dev(np.zeros((B, 3), F)), 1.0, return_normals=True)
    images, K, R, t = dev(S["images"]), dev(S["K"]), dev(S["R"]), dev(S["t"])
    vc = meshcolor.color_tsdf_mesh(m, images, K, R, t, SPHERE_MARGIN, min_cos=MIN_COS, return_flags=True)
    assert vc.color.shape == (m.verts.shape[0], 3) and vc.flags.shape == (m.verts.shape[0], V)
    # ... is the concatenation of per-track view_colors calls, bit for bit: by brute force, 'auto' and an explicit tree
    parts = {None: [], "auto": [], "tree": []}
    for b in range(B):
        verts, faces, normals = m.track(b)
        for how in parts:
            tree = renderer.MeshBVH(verts, faces) if how == "tree" else how
            parts[how].append(meshcolor.view_colors(verts, images[b], K, R[b], t[b], SPHERE_MARGIN, verts, faces, normals=normals,
                                                    min_cos=MIN_COS, bvh=tree, return_flags=True))
    got = [x.cpu().numpy() for x in (vc.color, vc.weight, vc.n_views, vc.flags)]
    for how, ps in parts.items():
        cat = [torch.cat([getattr(p, k) for p in ps]).cpu().numpy() for k in ("color", "weight", "n_views", "flags")]
        assert_same(got, cat, "color_tsdf_mesh against per-track calls (%s)" % how)
    monkeypatch.setattr(meshcolor, "AUTO_BVH_MIN_FACES", 256)                                      # 'auto' builds trees
    vt = meshcolor.color_tsdf_mesh(m, images, K, R, t, SPHERE_MARGIN, min_cos=MIN_COS, return_flags=True)
    monkeypatch.undo()
    assert_same([x.cpu().numpy() for x in (vt.color, vt.weight, vt.n_views, vt.flags)], got, "color_tsdf_mesh through trees")
    best = meshcolor.color_tsdf_mesh(m, images, K, R, t, SPHERE_MARGIN, min_cos=MIN_COS, mode="best")
    assert best.flags is None and same_bits(best.n_views.cpu().numpy(), got[2])
    color, n_views = got[0].astype(np.float64), got[2]
    v0 = 0
    for b in range(B):
        verts, faces, normals = (x.cpu().numpy() for x in m.track(b))
        nv = len(verts)
        assert len(faces) > 500
        X, N = verts.astype(np.float64), normals.astype(np.float64)
        centre, r = S["centres"][b], SPHERE_R[b]
        dr = np.abs(np.linalg.norm(X - centre, axis=1) - r).max()
        assert dr < 0.05                                                 # the mesh is the sphere: a property of the mesh
        tol = COLOR_TOL + 0.25 * GRAD_K * dr / MIN_COS
        facing = np.zeros(nv, bool)
        for v in range(V):
            R64, t64 = S["R"][b, v].astype(np.float64), S["t"][b, v].astype(np.float64)
            d = -R64.T @ t64 - X
            cosv = (N * d).sum(1) / np.linalg.norm(d, axis=1) / np.linalg.norm(N, axis=1)
            Sx = X @ R64.T + t64
            x, y = SPHERE_F * Sx[:, 0] / Sx[:, 2] + (W - 1) / 2.0, SPHERE_F * Sx[:, 1] / Sx[:, 2] + (H - 1) / 2.0
            assert x.min() > 1 and x.max() < W - 2 and y.min() > 1 and y.max() < H - 2     # the whole sphere is in the image
            facing |= cosv >= MIN_COS + 1e-3
        rows = slice(v0, v0 + nv)
        assert facing.sum() > nv // 3
        assert (n_views[rows][facing] >= 1).all()                        # every vertex facing a camera is coloured
        seen = n_views[rows] >= 1
        err = np.abs(color[rows][seen] - sphere_field(X[seen], centre)).max()
        print("track %d: %d vertices, %d coloured, dr %.4f, max |colour - g(X)| %.3e (tolerance %.3e)"
              % (b, nv, seen.sum(), dr, err, tol))
        assert err <= tol
        for name in ("best",):
            cb = best.color.cpu().numpy()[rows][seen].astype(np.float64)
            assert np.abs(cb - sphere_field(X[seen], centre)).max() <= tol
        # to_uint8 -> save_ply -> load_ply
        u8 = meshcolor.to_uint8(vc.color[rows], fill=(255, 0, 255))
        assert u8.dtype == torch.uint8 and u8.shape == (nv, 3)
        h8 = u8.cpu().numpy()
        assert (h8[~seen] == [255, 0, 255]).all()
        assert np.abs(h8[seen].astype(np.float64) - 255 * sphere_field(X[seen], centre)).max() <= 0.5 + 255 * tol
        path = str(tmp_path / ("track%d.ply" % b))
        mesh.save_ply(path, verts, faces, normals=normals, colors=u8)
        lv, lf, ln, lc = mesh.load_ply(path)
        assert same_bits(lv, verts) and np.array_equal(lf, faces) and same_bits(ln, normals) and np.array_equal(lc, h8)
        # the float colours go into the ray caster with the track's tree
        tv, tf, _ = m.track(b)
        bvh = renderer.MeshBVH(tv, tf)
        cols = torch.nan_to_num(vc.color[rows], nan=0.0).contiguous()
        Kh = S["K"]
        cam = renderer.PyCamera(Kh[0, 0], Kh[1, 1], Kh[0, 2], Kh[1, 2], S["R"][b, 0], S["t"][b, 0], W, H)
        proj = renderer.PyCamera(Kh[0, 0], Kh[1, 1], Kh[0, 2], Kh[1, 2], S["R"][b, 0], S["t"][b, 0] + np.array([-0.5, 0, 0], F),
                                 W, H)
        pattern = torch.ones((H, W, 3), dtype=torch.float32, device=DEV)
        depth, _, ambient = renderer.render_mesh_proj(tv, cols, tf, cam, proj, renderer.PyShader(1.0, 0.0, 0.0, 1.0), pattern,
                                                      bvh=bvh)
        hit = (depth > 0).cpu().numpy()
        amb = ambient.cpu().numpy().astype(np.float64)
        assert hit.sum() > 1000 and np.isfinite(amb).all()
        # with ka = 1 and kd = ks = 0 the ambient image is the interpolated vertex colour: the field again, where every
        # corner of the face was coloured (a pixel well inside the sphere's outline)
        yy, xx = np.nonzero(hit)
        inner = (xx - (W - 1) / 2.0) ** 2 + (yy - (H - 1) / 2.0) ** 2 < (0.5 * SPHERE_F * r / SPHERE_DIST) ** 2
        assert inner.sum() > 200
        R64, t64 = S["R"][b, 0].astype(np.float64), S["t"][b, 0].astype(np.float64)
        ray = np.stack([(xx - Kh[0, 2]) / Kh[0, 0], (yy - Kh[1, 2]) / Kh[1, 1], np.ones(len(xx))], 1) @ R64
        Xp = -R64.T @ t64 + depth.cpu().numpy()[yy, xx].astype(np.float64)[:, None] * ray
        diff = np.abs(amb[yy, xx] - sphere_field(Xp, centre))[inner].max()
        mix = 0.25 * GRAD_K ** 2 * 3.0 / 8                               # linear mix of g over a face of edges <= sqrt(3)
        print("track %d: rendered colours within %.3e of the field (tolerance %.3e)" % (b, diff, tol + mix))
        assert diff <= tol + mix                                         # vertex colours, then their barycentric mix
        v0 += nv
    assert v0 == m.verts.shape[0]
