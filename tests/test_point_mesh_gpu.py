"""GPU checks of the nearest-face query (ctd_point_mesh_distance_f32 of include/ctd_hip_mesh_dist.h, csrc/point_mesh.hip;
connecting_the_dots_amd.mesheval): the brute-force kernel bit for bit against the restatement tests/pointmesh_ref.py, the
BVH traversal bit for bit against the brute-force kernel on meshes and points built to break pruning, ties and the
clamp, and the reconstruction-error summary on meshes whose answers follow from their geometry."""
import functools

import numpy as np
import pytest
import torch

from tests import bvh_scenes, chain_scene
from tests import pointmesh_ref as pr

pytestmark = pytest.mark.gpu

DEV = "cuda"
F = np.float32
OK, UNSUPPORTED = 0, 3


def dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a, dtype).reshape(-1, 3)).to(DEV)


def raw(points, verts, faces, bvh=None, want_closest=True):
    """one call of the C entry point on device tensors -> (status, d2, face, closest) as numpy; the outputs start as
    garbage the kernel has to overwrite"""
    from connecting_the_dots_amd import _lib
    n = points.shape[0]
    d2 = torch.full((n,), -7.0, dtype=torch.float32, device=DEV)
    face = torch.full((n,), -7, dtype=torch.int32, device=DEV)
    closest = torch.full((n, 3), -7.0, dtype=torch.float32, device=DEV) if want_closest else None
    ptr = lambda t: t.data_ptr() if t is not None and t.numel() else None     # noqa: E731
    st = _lib.lib().ctd_point_mesh_distance_f32(
        ptr(points), n, ptr(verts), verts.shape[0], ptr(faces), faces.shape[0], None if bvh is None else bvh.buffer.data_ptr(),
        ptr(d2), ptr(face), ptr(closest), torch.cuda.current_device(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return st, d2.cpu().numpy(), face.cpu().numpy(), None if closest is None else closest.cpu().numpy()


def dsqrt(d2):
    """torch.sqrt on the device, as mesheval takes it"""
    return torch.sqrt(torch.from_numpy(np.ascontiguousarray(d2)).to(DEV)).cpu().numpy()


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    if a.dtype == np.float32:
        return bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())
    return bool(np.array_equal(a, b))


def assert_same(got, want, what):
    for name, g, w in zip(("d2", "face", "closest"), got, want):
        if not same_bits(g, w):
            bad = np.where((g != w).reshape(len(g), -1).any(1) & ~(np.isnan(g) & np.isnan(w)).reshape(len(g), -1).all(1))[0]
            raise AssertionError("%s: %s differs at %d of %d points, first %s: %s vs %s" % (
                what, name, len(bad), len(g), bad[:5], g[bad[:3]], w[bad[:3]]))


def both(points, verts, faces, what):
    """brute force and the traversal of a fresh tree on the same tensors, all three outputs bit for bit equal; -> the
    brute-force (d2, face, closest) and the tree"""
    from connecting_the_dots_amd import renderer
    p, v, f = dev(points, F), dev(verts, F), dev(faces, np.int32)
    bvh = renderer.MeshBVH(v, f)
    st, *ref = raw(p, v, f)
    assert st == OK
    st, *got = raw(p, v, f, bvh)
    if not bvh.usable:
        assert st == UNSUPPORTED
        return ref, bvh
    assert st == OK
    assert_same(got, ref, what)
    assert ref[1].min() >= -1 and ref[1].max() < max(len(f), 1)
    return ref, bvh


# ---------------------------------------------------------------------------------------------------------------------
# 1. the brute-force kernel is the restatement, bit for bit
# ---------------------------------------------------------------------------------------------------------------------
N_POINTS = (0, 1, 63, 64, 65, 1000)


def brute_mesh(n_faces):
    rs = np.random.RandomState(100 + n_faces)
    if n_faces > 1000:
        v, _, f = bvh_scenes.get_mesh_like(n_faces, 5)
        return v, f
    verts = rs.uniform(-1, 1, size=(max(3, 2 * n_faces), 3)).astype(F)
    faces = rs.randint(0, len(verts), size=(n_faces, 3)).astype(np.int32)     # a soup: shared and repeated vertices too
    if n_faces == 257:                                    # indices outside [0, n_verts): skipped, never dereferenced
        faces[[3, 100, 256]] = [[-1, 0, 1], [0, len(verts), 1], [2, 3, 1 << 30]]
        faces[0] = faces[1]
    return verts, faces


def brute_points(verts, rs):
    n = N_POINTS[-1]
    near = verts[rs.randint(0, len(verts), n // 2)] + rs.normal(size=(n // 2, 3)) * 1e-3
    near[:50] = verts[rs.randint(0, len(verts), 50)]                           # exactly on vertices
    return np.concatenate([near, rs.uniform(-3, 3, size=(n - n // 2, 3)) + [0, 0, 2]]).astype(F)


@pytest.mark.parametrize("n_faces", [0, 1, 5, 257, 2000])
def test_brute_force_is_the_restatement(n_faces):
    verts, faces = brute_mesh(n_faces)
    pts = brute_points(verts, np.random.RandomState(n_faces))
    want = pr.nearest(pts, verts, faces)                                       # once, for the 1000 points
    assert n_faces == 0 or (want[1] >= 0).all()
    v, f = dev(verts, F), dev(faces, np.int32)
    for n in N_POINTS:
        st, *got = raw(dev(pts[:n], F), v, f)
        assert st == OK
        assert_same(got, [w[:n] for w in want], "%d faces, %d points" % (len(faces), n))
    st, d2, face, closest = raw(dev(pts, F), v, f, want_closest=False)         # closest is optional
    assert st == OK and closest is None and same_bits(d2, want[0]) and same_bits(face, want[1])
    if n_faces == 0:
        assert (want[1] == -1).all() and np.isposinf(want[0]).all() and np.isnan(want[2]).all()


# ---------------------------------------------------------------------------------------------------------------------
# 2. the traversal is the brute-force kernel, bit for bit
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def scene2000():
    v, _, f = bvh_scenes.get_mesh_like(2000, 5)
    return v, f


def test_bvh_near_and_far_points():
    v, f = scene2000()
    rs = np.random.RandomState(1)
    near = (v[6:] + rs.normal(size=v[6:].shape) * 1e-3).astype(F)
    ref, bvh = both(near, v, f, "near the surface")
    assert bvh.usable and (np.sqrt(ref[0]) < 0.02).all()
    far = (rs.normal(size=(1000, 3)) * 1e3).astype(F)
    both(far, v, f, "far away")
    both(np.array([[1e4, 1e4, 1e4], [-1e4, 0, 2], [0, 0, 1e4], [3e4, -2e4, 1e4]], F), v, f, "all faces nearly equidistant")
    both((near[::3].astype(np.float64) + 1e3).astype(F), (v.astype(np.float64) + 1e3).astype(F), f, "translated by 1e3")


def grid_mesh(n=16):
    ys, xs = np.meshgrid(np.arange(n + 1), np.arange(n + 1), indexing="ij")
    verts = np.stack([xs, ys, np.zeros_like(xs)], -1).reshape(-1, 3).astype(F) / 8
    i, j = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    a = (i * (n + 1) + j).reshape(-1)
    faces = np.concatenate([np.stack([a, a + 1, a + n + 2], 1), np.stack([a, a + n + 2, a + n + 1], 1)])
    return verts, faces.astype(np.int32)


def test_bvh_points_on_vertices_edges_and_faces_of_a_grid():
    verts, faces = grid_mesh()
    a, b, c = (verts[faces[:, k]] for k in range(3))
    pts = np.concatenate([verts, (a + b) / 2, (b + c) / 2, (a + c) / 2, (a + b) / 4 + c / 2,
                          verts + [0, 0, 0.5], (a + b) / 2 + [0, 0, -0.25]]).astype(F)
    ref, _ = both(pts, verts, faces, "on the grid")
    on = len(pts) - len(verts) - len(a)
    assert (ref[0][:on] == 0).all()                       # dyadic coordinates: exactly on the mesh
    want = pr.nearest(pts, verts, faces)
    assert_same(ref, want, "grid against the restatement")
    # a vertex is shared by up to six faces, an edge by two: the lowest index wins
    first_with = np.full(len(verts), len(faces))
    for k in range(3):
        np.minimum.at(first_with, faces[:, k], np.arange(len(faces)))
    assert np.array_equal(ref[1][:len(verts)], first_with)


def test_bvh_duplicate_and_coplanar_faces():
    rs = np.random.RandomState(2)
    quad = np.array([[-1, -1, 2], [1, -1, 2], [1, 1, 2], [-1, 1, 2]], F)
    verts = np.concatenate([quad, quad * [0.5, 0.5, 1], quad * [1.5, 1.5, 1]]).astype(F)
    base = np.array([[0, 1, 2], [0, 2, 3]])
    faces = np.concatenate([base, base + 4, base, base + 8, base + 4, base[::-1]] * 3)
    pts = np.concatenate([rs.uniform(-2, 2, size=(500, 3)) + [0, 0, 2], verts, rs.uniform(-1, 1, size=(200, 3)) * [1, 1, 0] +
                          [0, 0, 2]]).astype(F)
    ref, _ = both(pts, verts, faces, "duplicates")
    assert (ref[1] < 10).all()                            # every later copy loses its ties


def test_bvh_degenerate_and_nonfinite_faces_and_points():
    rs = np.random.RandomState(5)
    v, f = bvh_scenes.icosphere(2)
    v = (v * 0.5 + [0, 0, 2]).astype(F)
    bad = np.array([[np.nan, 0, 2], [np.inf, 0, 2], [0, -np.inf, 2], [0.1, 0.1, 1.5], [0.1, 0.1, 1.5],
                    [0.2, 0.2, 1.5], [1e30, 1e30, 2], [-1e30, 1e30, 2], [0.3, 0.3, 1.5], [3e38, 0, 0]], F)
    verts = np.concatenate([v, bad]).astype(F)
    n = len(v)
    extra = np.array([[n, 0, 1], [n + 1, 2, 3], [n + 2, 4, 5], [n + 3, n + 4, n + 5], [n + 3, n + 3, n + 3],
                      [n + 6, n + 7, 6], [0, 1, n + 1], [n + 3, n + 5, n + 8], [n + 5, n + 5, n + 3], [0, 0, 1], [5, 5, 5],
                      [n + 9, 7, 8]])
    faces = np.concatenate([extra[:3], f, extra[3:]])
    pts = np.concatenate([rs.uniform(-1, 1, size=(600, 3)) + [0, 0, 2], verts[np.abs(verts).max(1) < 100],
                          [[0.15, 0.15, 1.5], [0.25, 0.25, 1.5], [0.1, 0.1, 1.4]]]).astype(F)
    ref, _ = both(pts, verts, faces, "degenerate and non-finite faces")
    assert_same(ref, pr.nearest(pts, verts, faces), "degenerate faces against the restatement")
    assert (ref[1] >= 0).all()
    weird = np.array([[np.nan, 0, 2], [0, np.inf, 2], [-np.inf, np.nan, 0], [1e30, 0, 0], [3e38, 3e38, 3e38], [0, 0, 2]], F)
    ref, _ = both(weird, verts, faces, "non-finite points")
    assert ref[1][:5].tolist() == [-1] * 5 and np.isposinf(ref[0][:5]).all() and np.isnan(ref[2][:5]).all() and ref[1][5] >= 0
    nanv = np.full((30, 3), np.nan, F)
    ref, _ = both(pts[:100], nanv, np.arange(30).reshape(-1, 3), "an all-NaN mesh")
    assert (ref[1] == -1).all() and np.isposinf(ref[0]).all() and np.isnan(ref[2]).all()


def test_bvh_board_and_tiny_faces():
    """the data generator's 1000-unit board (two faces) over a field of faces a millionth of its size"""
    rs = np.random.RandomState(6)
    board = np.array([[-500, -500, 3], [500, -500, 3], [500, 500, 3], [-500, -500, 3], [500, 500, 3], [-500, 500, 3]], F)
    centres = rs.uniform(-2, 2, size=(400, 1, 3)) + [0, 0, 2]
    tiny = (centres + rs.normal(size=(400, 3, 3)) * 1e-3).reshape(-1, 3)
    verts = np.concatenate([board, tiny]).astype(F)
    faces = np.arange(len(verts)).reshape(-1, 3)
    pts = np.concatenate([centres[:, 0] + rs.normal(size=(400, 3)) * 1e-3, rs.uniform(-3, 3, size=(300, 3)) + [0, 0, 2],
                          rs.uniform(-400, 400, size=(300, 3)) * [1, 1, 0.01] + [0, 0, 3]]).astype(F)
    ref, bvh = both(pts, verts, faces, "board and tiny faces")
    assert bvh.usable and (ref[1][-300:] < 2).mean() > 0.9 and (ref[1][:400] >= 2).mean() > 0.9


def test_bvh_fuzz():
    """20 seeded meshes of 50-3000 random faces, 512 points each: soups and index-sharing meshes, scales 1e-3..10"""
    for seed in range(20):
        rs = np.random.RandomState(2000 + seed)
        n = int(rs.randint(50, 3001))
        scale = 10.0 ** rs.uniform(-3, 1)
        centre = rs.normal(size=3) * [1, 1, 2]
        if seed % 2:
            cs_ = centre + rs.normal(size=(n, 1, 3)) * scale * 10
            verts = (cs_ + rs.normal(size=(n, 3, 3)) * scale).reshape(-1, 3).astype(F)
            faces = np.arange(3 * n).reshape(-1, 3)
        else:
            verts = (centre + rs.normal(size=(n, 3)) * scale).astype(F)
            faces = rs.randint(0, n, size=(n, 3))
        pts = np.concatenate([verts[rs.randint(0, len(verts), 256)] + rs.normal(size=(256, 3)) * scale * 1e-2,
                              centre + rs.normal(size=(256, 3)) * scale * 30]).astype(F)
        both(pts, verts, faces, "fuzz seed %d (%d faces)" % (seed, n))


def test_two_calls_give_identical_bytes():
    from connecting_the_dots_amd import renderer
    v, f = scene2000()
    pts = (v[6:] + np.random.RandomState(3).normal(size=v[6:].shape) * 1e-2).astype(F)
    p, vt, ft = dev(pts, F), dev(v, F), dev(f, np.int32)
    bvh = renderer.MeshBVH(vt, ft)
    for tree in (None, bvh):
        a, b = raw(p, vt, ft, tree), raw(p, vt, ft, tree)
        assert a[0] == b[0] == OK
        assert_same(a[1:], b[1:], "second call")


def deep_mesh():
    """the chain of tests/test_render_bvh_gpu.test_deep_trees_render_identically_or_fall_back: one centroid per Morton bit"""
    pts = []
    for p in range(62, -1, -1):
        q = [0.0, 0.0, 0.0]
        q[2 - p % 3] = float(2 ** (p // 3))
        for _ in range(4):
            pts.append(q)
    pts += [[0.0, 0.0, 0.0]] * 64
    pts = np.array(pts, np.float64) * 1e-5 + [0, 0, 1]
    tri = np.array([[0, 0, 0], [1e-3, 0, 0], [0, 1e-3, 0]])
    verts = (pts[:, None, :] + tri[None]).reshape(-1, 3).astype(F)
    return verts, np.arange(len(verts)).reshape(-1, 3)


def test_deep_tree_gives_identical_results_or_falls_back():
    from connecting_the_dots_amd import mesheval
    verts, faces = deep_mesh()
    rs = np.random.RandomState(8)
    pts = np.concatenate([verts[::5] + rs.normal(size=verts[::5].shape) * 1e-4, rs.uniform(-1, 1, size=(200, 3)) + [0, 0, 1]])
    ref, bvh = both(pts.astype(F), verts, faces, "deep tree")         # identical, or UNSUPPORTED from the C call
    assert bvh.usable == (bvh.depth <= 62)
    p = dev(pts, F)
    dist, face = mesheval.point_mesh_distance(p, bvh.verts, bvh.faces, bvh=bvh)   # usable or not: the same answer
    assert same_bits(face.cpu().numpy(), ref[1]) and same_bits(dist.cpu().numpy(), dsqrt(ref[0]))
    same = np.tile(np.array([[-0.5, -0.5, 2], [0.5, -0.5, 2], [0, 0.5, 2]], F), (300, 1))
    ref, bvh = both(pts.astype(F), same, np.arange(900).reshape(-1, 3), "300 copies of one face")
    assert bvh.usable and (ref[1] == 0).all()


# ---------------------------------------------------------------------------------------------------------------------
# 3. the Python module
# ---------------------------------------------------------------------------------------------------------------------
def test_auto_none_and_an_explicit_tree_agree(monkeypatch):
    from connecting_the_dots_amd import mesheval, renderer
    v, f = scene2000()
    pts = (v[6:] + np.random.RandomState(4).normal(size=v[6:].shape) * 1e-2).astype(F)
    p, vt, ft = dev(pts, F), dev(v, F), dev(f, np.int32)
    want = pr.nearest(pts, v, f)
    built = []
    real = renderer.MeshBVH
    outs = [mesheval.point_mesh_distance(p, vt, ft, bvh=None, return_closest=True)]
    outs.append(mesheval.point_mesh_distance(p, vt, ft, bvh=real(vt, ft), return_closest=True))
    monkeypatch.setattr(renderer, "MeshBVH", lambda *a, **k: built.append(1) or real(*a, **k))     # counts 'auto' builds
    outs.append(mesheval.point_mesh_distance(p, vt, ft, bvh="auto", return_closest=True))
    assert len(built) == (len(f) >= mesheval.AUTO_BVH_MIN_FACES)
    monkeypatch.setattr(mesheval, "AUTO_BVH_MIN_FACES", 1024)
    outs.append(mesheval.point_mesh_distance(p, vt, ft, bvh="auto", return_closest=True))      # above it: builds
    assert len(built) >= 1
    monkeypatch.undo()
    for dist, face, closest in outs:
        assert dist.dtype == torch.float32 and face.dtype == torch.int32 and closest.shape == (len(pts), 3)
        assert same_bits(face.cpu().numpy(), want[1]) and same_bits(closest.cpu().numpy(), want[2])
        assert same_bits(dist.cpu().numpy(), dsqrt(want[0]))
    assert len(mesheval.point_mesh_distance(p, vt, ft)) == 2
    bad = ft.clone()
    bad[7, 1] = len(v)                                                # 'auto' must not hand such faces to the tree's build
    dist, face = mesheval.point_mesh_distance(p, vt, bad, bvh="auto")
    assert same_bits(face.cpu().numpy(), pr.nearest(pts, v, bad.cpu().numpy())[1])
    with pytest.raises(RuntimeError, match="other verts / faces"):
        mesheval.point_mesh_distance(p, vt, ft, bvh=real(vt.clone(), ft))
    with pytest.raises(RuntimeError, match="unsupported dtype"):
        mesheval.point_mesh_distance(p.double(), vt, ft)
    with pytest.raises(RuntimeError, match="unsupported dtype"):
        mesheval.point_mesh_distance(p, vt, ft.long())
    with pytest.raises(RuntimeError, match=r"shaped \[n,3\]"):
        mesheval.point_mesh_distance(p.reshape(-1), vt, ft)
    with pytest.raises(RuntimeError, match="contiguous"):
        mesheval.point_mesh_distance(p[:, [2, 1, 0]].t().contiguous().t(), vt, ft)
    empty = mesheval.point_mesh_distance(p[:0], vt, ft, return_closest=True)
    assert [tuple(t.shape) for t in empty] == [(0,), (0,), (0, 3)]


def test_chain_scene_truth_points_lie_on_their_mesh():
    sc = chain_scene.scene()
    from connecting_the_dots_amd import mesheval
    meshes = [(dev(m["verts"], F), dev(m["faces"], np.int32)) for m in sc.meshes]
    for b in range(chain_scene.B):
        T = sc.truth[b][0]
        X = T["X"][T["hit"]][::7]
        pts = X.astype(F)
        m = sc.meshes[b]
        d64 = chain_scene.mesh_distance(pts, m["verts"], m["faces"])            # of the rounded points: <= u |X| sqrt(3)
        assert d64.max() <= pr.U * np.linalg.norm(X, axis=1).max() * 3 ** 0.5
        face64 = pr.nearest(pts, m["verts"], m["faces"], np.float64)[1]
        tol = pr.forward_bound(pts, m["verts"], m["faces"], face64, d64)
        own, _ = mesheval.point_mesh_distance(dev(pts, F), *meshes[b], bvh="auto")
        own = own.cpu().numpy().astype(np.float64)
        print("track %d: %d truth points at most %.3e from their mesh (allowed %.3e)" % (b, len(pts), own.max(), tol.max()))
        assert (np.abs(own - d64) <= tol).all()
        o = sc.meshes[1 - b]
        other64 = chain_scene.mesh_distance(pts, o["verts"], o["faces"])
        other, _ = mesheval.point_mesh_distance(dev(pts, F), *meshes[1 - b])
        other = other.cpu().numpy().astype(np.float64)
        tol_o = pr.forward_bound(pts, o["verts"], o["faces"], pr.nearest(pts, o["verts"], o["faces"], np.float64)[1], other64)
        assert (np.abs(other - other64) <= tol_o).all()
        assert other64.min() > 0.1 and other.min() > 0.1 > 100 * own.max()       # far from the other track's mesh


@functools.lru_cache(maxsize=None)
def sphere3():
    v, f = bvh_scenes.icosphere(3)
    return v.astype(F), f.astype(np.int32)


def test_reconstruction_error_of_identical_meshes_is_zero():
    from connecting_the_dots_amd import mesheval
    v, f = sphere3()
    vt, ft = dev(v, F), dev(f, np.int32)
    for bvh in (None, "auto"):
        e = mesheval.reconstruction_error(vt, ft, vt.clone(), ft.clone(), thresholds=(0.0, 1e-3), bvh=bvh)
        for side in ("accuracy", "completeness"):
            s = e[side]
            assert s["mean"] == s["rms"] == s["median"] == s["max"] == 0.0 and s["within"] == [1.0, 1.0]
            assert s["n"] == len(v) and s["n_unmatched"] == 0
        assert e["chamfer"] == 0.0 and e["fscore"] == [1.0, 1.0] and e["n_unmatched"] == 0 and e["thresholds"] == [0.0, 1e-3]


def test_reconstruction_error_of_a_scaled_sphere():
    from connecting_the_dots_amd import mesheval
    v, f = sphere3()
    big = (v.astype(np.float64) * 1.01).astype(F)
    # t: the largest angle between a face's normal and one of its corners; the faces dip below the sphere by at most
    # the sagitta 1 - cos(t).  Outwards: a vertex 1.01 v is 0.01 from v, a vertex of the inner mesh, and at least 0.01
    # from the unit ball that contains it.  Inwards: v is 0.01 from 1.01 v, and its distance to the plane of a face of
    # the larger mesh that has 1.01 v as a corner is n.(1.01 v) - n.v = 0.01 cos(angle) >= 0.01 cos(t); the other faces
    # are farther.  So every distance, either way, lies in [0.01 cos(t), 0.01 + sagitta].
    a, b, c = (v.astype(np.float64)[f[:, k]] for k in range(3))
    nrm = np.cross(b - a, c - a)
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    cos_t = min((nrm * a).sum(1).min(), (nrm * b).sum(1).min(), (nrm * c).sum(1).min())
    sagitta = 1 - cos_t
    lo, hi = 0.01 * cos_t, 0.01 + sagitta
    vt, ft, bt = dev(v, F), dev(f, np.int32), dev(big, F)
    dist, _ = mesheval.point_mesh_distance(bt, vt, ft)
    dist = dist.cpu().numpy().astype(np.float64)
    # the rounding of the vertices (|v| = 1 and 1.01 v, 2u each) and the kernel's own error, bound (2) / (3)
    d2_64, face64, _ = pr.nearest(big, v, f, np.float64)
    slack = 4 * pr.U * 1.01 + pr.forward_bound(big, v, f, face64, np.sqrt(d2_64)).max()
    print("scaled sphere: distances %.6f .. %.6f, allowed %.6f .. %.6f" % (dist.min(), dist.max(), lo, hi))
    assert dist.min() >= lo - slack and dist.max() <= hi + slack
    e = mesheval.reconstruction_error(bt, ft, vt, ft, thresholds=(0.005, 0.05))
    assert lo - slack <= e["accuracy"]["mean"] <= e["accuracy"]["max"] <= hi + slack
    assert e["accuracy"]["within"] == [0.0, 1.0] and e["completeness"]["within"] == [0.0, 1.0]
    assert e["fscore"] == [0.0, 1.0] and e["n_unmatched"] == 0
    assert abs(e["chamfer"] - (e["accuracy"]["mean"] + e["completeness"]["mean"])) < 1e-15
    assert e["accuracy"]["mean"] <= e["accuracy"]["rms"] <= e["accuracy"]["max"]


def test_reconstruction_error_with_half_the_faces_removed():
    from connecting_the_dots_amd import mesheval
    v, f = sphere3()
    cen = v.astype(np.float64)[f].mean(1)
    keep = f[cen[:, 2] >= 0]
    a, b, c = (v.astype(np.float64)[f[:, k]] for k in range(3))
    area = 0.5 * np.linalg.norm(np.cross(b - a, c - a), axis=1)
    share = area[cen[:, 2] >= 0].sum() / area.sum()
    vt, ft, kt = dev(v, F), dev(f, np.int32), dev(keep, np.int32)
    g = torch.Generator(device=DEV)
    g.manual_seed(123)
    n = 20000
    e = mesheval.reconstruction_error(vt, kt, vt, ft, thresholds=(1e-4,), n_samples=n, generator=g)
    # a sample of a kept face lies on the truth mesh up to its own rounding, 4u (|a| + |b| + |c|), and the kernel's
    # error by (2) / (3) with R <= E (the point is on the face): 2 (eta + 47.5u E^5 / A^2 + 16u E^2 / e_min)
    E = max(np.linalg.norm(b - a, axis=1).max(), np.linalg.norm(c - a, axis=1).max())
    e_min = min(np.linalg.norm(b - a, axis=1).min(), np.linalg.norm(c - a, axis=1).min(), np.linalg.norm(c - b, axis=1).min())
    on_mesh = 12 * pr.U + 2 * (pr.eta(v, f).max() + 47.5 * pr.U * E ** 5 / area.min() ** 2 + 16 * pr.U * E ** 2 / e_min)
    print("half sphere: accuracy max %.3e, allowed %.3e" % (e["accuracy"]["max"], on_mesh))
    assert on_mesh < 1e-4
    assert e["accuracy"]["max"] <= on_mesh and e["accuracy"]["within"] == [1.0] and e["accuracy"]["n"] == n
    sigma = (share * (1 - share) / n) ** 0.5
    got = e["completeness"]["within"][0]
    print("half sphere: completeness within 1e-4 %.4f, area share %.4f +- %.4f" % (got, share, 4 * sigma))
    # a truth sample over a removed face is >= 1e-4 from the kept half except in a strip of that width along the cut:
    # at most 1e-4 * (the cut's length <= 2 pi) / (4 pi) of the area, far below sigma
    assert abs(got - share) <= 4 * sigma + 1e-4
    g.manual_seed(123)
    again = mesheval.reconstruction_error(vt, kt, vt, ft, thresholds=(1e-4,), n_samples=n, generator=g)
    assert again == e
    e2 = mesheval.reconstruction_error(vt, kt, vt, ft, thresholds=(1e-4,))      # vertices: accuracy exactly 0
    assert e2["accuracy"]["max"] == 0.0 and 0.4 < e2["completeness"]["within"][0] < 0.7
