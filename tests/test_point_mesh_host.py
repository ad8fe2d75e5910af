"""CPU-only checks of the nearest-face query (include/ctd_hip_mesh_dist.h: ctd_point_mesh_distance_f32;
connecting_the_dots_amd.mesheval): the rule's sentences (the header against its ctypes table: tests/test_abi_and_host.py),
argument validation before any HIP call, the Python module's own rejections, the restatement tests/pointmesh_ref.py against
hand-made answers and against the float64 reference tests/chain_scene.mesh_distance, and sample_surface on CPU tensors.

Restatement (numpy f32) against chain_scene.mesh_distance (float64, formulated differently), 500 points each, measured
max |sqrt(d2) - d64| and the smallest / largest allowed value, pointmesh_ref.forward_bound (the bound (2) / (3) of
csrc/point_mesh.hip evaluated per point):
  icosphere(2), 320 faces, points in the box +- 1.5:         7.8e-08, allowed 5.4e-06 .. 2.7e-04
  get_mesh_like(500, 3), 340 faces with the 1000-unit board: 5.1e-06, allowed 1.9e-03 .. 3.6e-02
  get_mesh_like(500, 4), 340 faces with the board:           3.1e-07, allowed 1.9e-03 .. 3.6e-02
(points uniform in the objects' bounding box grown by 0.5).  The bound is loose because (3) is a worst case over slivers
and the board's coordinates reach 500 (one ulp there is 3e-5, and the board's eta alone is 9.5e-4); it is derived, not
tuned.  The float64 run of the same restatement agrees with mesh_distance to 6e-16."""
import os

import numpy as np
import pytest
import torch

from tests import bvh_scenes, chain_scene
from tests import pointmesh_ref as pr
from tests.test_tsdf_host import _Bufs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIST_HEADER = os.path.join(ROOT, "include", "ctd_hip_mesh_dist.h")
OK, INVALID_ARG = 0, 1
F = np.float32


@pytest.fixture(scope="module")
def L():
    from connecting_the_dots_amd import _lib
    return _lib.lib()


# ---------------------------------------------------------------------------------------------------------------------
# 1. the header (header == ctypes table == exports: tests/test_abi_and_host.py, for every header)
# ---------------------------------------------------------------------------------------------------------------------
def test_the_header_states_the_rule():
    text = " ".join(open(DIST_HEADER).read().replace("*", " ").split())
    for phrase in ("One function computes the distance",
                   "It works in f32, in one fixed operation order, with no contracted multiply-adds",
                   "It classifies by region, as Ericson's closest point on a triangle does",
                   "A vertex region returns that vertex itself",
                   "Every other region clamps the two parameters after classification",
                   "so a NaN parameter becomes 0",
                   "a convex combination of a, a + ab and a + ac whatever rounding did to the region tests",
                   "d2 = dx dx + dy dy + dz dz with d = p - q, summed in that order",
                   "the face of smallest d2 among the faces whose d2 compares < +inf",
                   "so a NaN or overflowed d2 never wins",
                   "On equal d2 the lowest face index wins",
                   "If no face qualifies: face = -1, d2 = +inf, closest = NaN",
                   "Faces with an index outside [0, n_verts) are skipped and never dereferenced on the brute-force path",
                   "Degenerate faces are ordinary faces",
                   "The kernel outputs d2, not the distance",
                   "The same bits on every run and on both paths",
                   "One lane owns one point: no atomics",
                   "this kernel is the definition",
                   "A point with a non-finite coordinate prunes nothing",
                   "nodes with infinite boxes (faces with non-finite vertices) are never pruned",
                   "CTD_ERR_UNSUPPORTED for a tree deeper than the traversal stack",
                   "n_points == 0 is CTD_OK and does nothing",
                   'n_faces == 0 is CTD_OK and fills the answer of "no face qualifies"'):
        assert phrase in text, phrase


# ---------------------------------------------------------------------------------------------------------------------
# 2. validation before any HIP call
# ---------------------------------------------------------------------------------------------------------------------
def test_rejections_need_no_gpu(L):
    bufs = _Bufs(["points", "verts", "faces", "bvh", "d2", "face", "closest"])

    def call(n=10, nv=10, nf=10, **ptrs):
        p = dict(bufs.ptr, **ptrs)
        return L.ctd_point_mesh_distance_f32(p["points"], n, p["verts"], nv, p["faces"], nf, p["bvh"], p["d2"], p["face"],
                                             p["closest"], -1, None)

    for kw in (dict(n=-1), dict(nv=-1), dict(nf=-1), dict(points=None), dict(d2=None), dict(face=None), dict(verts=None),
               dict(faces=None), dict(bvh=bufs.ptr["bvh"] + 4), dict(bvh=bufs.ptr["bvh"] + 8),
               dict(n=(1 << 31) // 3 + 1), dict(nf=(1 << 28) + 1), dict(n=-1, bvh=None), dict(faces=None, bvh=None),
               dict(n=0, nf=-1), dict(n=0, bvh=bufs.ptr["bvh"] + 4)):
        assert call(**kw) == INVALID_ARG, kw
    # nothing to do: CTD_OK before any HIP call, with or without a tree, closest and the mesh's pointers NULL or not
    assert call(n=0) == OK and call(n=0, bvh=None, closest=None) == OK
    assert call(n=0, points=None, d2=None, face=None, nf=0, verts=None, faces=None) == OK


def _fake_bvh(verts, faces, usable=True):
    from connecting_the_dots_amd import renderer
    b = renderer.MeshBVH.__new__(renderer.MeshBVH)                   # the build needs a GPU; `matches` and `usable` do not
    b.verts, b.faces, b.usable = verts, faces, usable
    return b


def test_mesheval_rejections_need_no_gpu():
    from connecting_the_dots_amd import _meshargs, mesheval
    resolve = lambda *a: _meshargs._resolve_bvh(*a, mesheval.AUTO_BVH_MIN_FACES)      # noqa: E731  as point_mesh_distance calls it
    assert sorted(n for n in vars(mesheval) if not n.startswith("_") and
                  getattr(getattr(mesheval, n), "__module__", "") == mesheval.__name__) == [
        "point_mesh_distance", "reconstruction_error", "sample_surface"]
    p, v = torch.zeros(4, 3), torch.zeros(5, 3)
    f = torch.zeros(2, 3, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="CUDA tensor"):
        mesheval.point_mesh_distance(p, v, f)
    with pytest.raises(RuntimeError, match="CUDA tensor"):
        mesheval.reconstruction_error(v, f, v, f, (0.1,))
    with pytest.raises(RuntimeError, match="must be a tensor"):
        mesheval.point_mesh_distance(p.numpy(), v, f)
    # (the shared argument check looks at the device before the dtype: wrong dtypes of CUDA tensors are refused in
    # tests/test_point_mesh_gpu.py, wrong dtypes of CPU tensors by sample_surface below, wrong shapes in the next test)
    # a tree of other tensors, an unusable tree, a wrong kind of bvh
    other_v, other_f = v.clone(), f.clone()
    with pytest.raises(RuntimeError, match="other verts / faces"):
        resolve(_fake_bvh(other_v, f), v, f, "point_mesh_distance")
    with pytest.raises(RuntimeError, match="other verts / faces"):
        resolve(_fake_bvh(v, other_f), v, f, "point_mesh_distance")
    with pytest.raises(RuntimeError, match="other verts / faces"):
        resolve(_fake_bvh(v, f), v[:4], f, "point_mesh_distance")
    for bad in ("bvh", 3, (v, f)):
        with pytest.raises(RuntimeError, match="None, 'auto' or a renderer.MeshBVH"):
            resolve(bad, v, f, "point_mesh_distance")
    good = _fake_bvh(v, f)
    assert resolve(good, v, f, "x") is good and resolve(None, v, f, "x") is None
    assert resolve(_fake_bvh(v, f, usable=False), v, f, "x") is None       # falls back to brute force
    assert resolve("auto", v, f, "x") is None                               # below the threshold: no build
    t = mesheval.AUTO_BVH_MIN_FACES
    assert t >= 2 and t & (t - 1) == 0                                                   # a power of two


def test_shape_rejections_on_the_argument_helper():
    import unittest.mock as mock
    from connecting_the_dots_amd import _meshargs
    with mock.patch.object(_meshargs, "_check", lambda *a, **k: None):    # the device check comes first: step over it
        for bad in (torch.zeros(4), torch.zeros(4, 2), torch.zeros(2, 4, 3)):
            with pytest.raises(RuntimeError, match=r"must be shaped \[n,3\]"):
                _meshargs._nx3(bad, "point_mesh_distance", "points", torch.float32)
        assert _meshargs._nx3(torch.zeros(0, 3), "w", "points", torch.float32).shape == (0, 3)


# ---------------------------------------------------------------------------------------------------------------------
# 3. the restatement against hand-made answers
# ---------------------------------------------------------------------------------------------------------------------
TRI = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], F)


def test_one_point_in_each_of_the_seven_regions():
    pts = np.array([[-1, -1, 0.5], [2, -0.5, 0], [-0.5, 2, 0], [0.5, -1, 0], [-1, 0.5, 0], [1, 1, 0], [0.25, 0.25, 2]], F)
    want_q = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0.5, 0, 0], [0, 0.5, 0], [0.5, 0.5, 0], [0.25, 0.25, 0]], F)
    want_d2 = np.array([2.25, 1.25, 1.25, 1.0, 1.0, 0.5, 4.0], F)
    d2, face, q = pr.nearest(pts, TRI, np.array([[0, 1, 2]]))
    assert d2.dtype == F and q.dtype == F and face.dtype == np.int32
    assert np.array_equal(d2, want_d2) and np.array_equal(q, want_q) and (face == 0).all()
    # the corners themselves, in any role, are at distance 0 exactly -- also with coordinates that do not subtract exactly
    rs = np.random.RandomState(0)
    tri = (rs.normal(size=(3, 3)) * [1, 10, 100]).astype(F)
    for perm in ([0, 1, 2], [1, 2, 0], [2, 0, 1], [0, 2, 1]):
        d2, face, q = pr.nearest(tri, tri, np.array([perm]))
        assert np.array_equal(d2, np.zeros(3, F)) and np.array_equal(q, tri)


def test_ties_go_to_the_lower_index_and_nothing_qualifies_on_a_nan_mesh():
    verts = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0]], F)
    faces = np.array([[2, 1, 3], [0, 1, 2], [0, 1, 2], [1, 0, 2]])
    pts = np.array([[0.5, 0.5, 0], [0.25, 0.25, 1], [0.75, 0.75, 0.5], [1, 0, 0]], F)
    d2, face, q = pr.nearest(pts, verts, faces)
    assert face.tolist() == [0, 1, 0, 0]              # the shared edge; the duplicated face; only face 0; a shared vertex
    assert np.array_equal(d2, np.array([0, 1, 0.25, 0], F))
    d2, face, q = pr.nearest(pts, verts, faces[::-1])
    assert face.tolist() == [0, 0, 3, 0]
    # faces with an index out of range take no part; a NaN vertex poisons only its faces
    bad = np.array([[0, 1, 4], [-1, 1, 2], [0, 1, 2]])
    assert pr.nearest(pts, verts, bad)[1].tolist() == [2, 2, 2, 2]
    nanv = verts.copy()
    nanv[3] = np.nan
    assert pr.nearest(pts, nanv, faces)[1].tolist() == [1, 1, 1, 1]
    d2, face, q = pr.nearest(pts, np.full((4, 3), np.nan, F), faces)
    assert (face == -1).all() and np.isposinf(d2).all() and np.isnan(q).all()
    d2, face, q = pr.nearest(pts, verts, np.zeros((0, 3), np.int64))
    assert (face == -1).all() and np.isposinf(d2).all() and np.isnan(q).all()
    d2, face, q = pr.nearest(np.full((1, 3), 1e30, F), verts, faces)                       # d2 overflows: never wins
    assert face[0] == -1 and np.isposinf(d2[0])
    # zero-area faces are ordinary faces: the computed point is a convex combination of the corners, d2 finite
    deg = np.array([[0, 0, 0], [1, 0, 0], [2, 0, 0], [3, 3, 3]], F)
    d2, face, q = pr.nearest(pts, deg, np.array([[0, 1, 2], [3, 3, 3], [0, 0, 1]]))
    assert np.isfinite(d2).all() and (face >= 0).all() and (q[:, 0] >= 0).all() and (q[:, 0] <= 3).all()


# ---------------------------------------------------------------------------------------------------------------------
# 4. the restatement against the float64 reference
# ---------------------------------------------------------------------------------------------------------------------
def _scene(name):
    if name == "icosphere":
        v, f = bvh_scenes.icosphere(2)
        return v.astype(F), f.astype(np.int64), np.array([-1.5] * 3), np.array([1.5] * 3)
    v, _, f = bvh_scenes.get_mesh_like(500, int(name))
    obj = v[6:]                                                      # the objects; the board's corners are the first six
    return v, f.astype(np.int64), obj.min(0) - 0.5, obj.max(0) + 0.5


@pytest.mark.parametrize("name", ["icosphere", "3", "4"])
def test_restatement_against_float64(name):
    v, f, lo, hi = _scene(name)
    pts = np.random.RandomState(7).uniform(lo, hi, size=(500, 3)).astype(F)
    d2, face, q = pr.nearest(pts, v, f)
    d2d, face64, _ = pr.nearest(pts, v, f, np.float64)
    d64 = chain_scene.mesh_distance(pts, v, f)
    assert np.abs(np.sqrt(d2d) - d64).max() < 1e-12                 # two formulations, both float64
    err = np.abs(np.sqrt(d2.astype(np.float64)) - d64)
    tol = pr.forward_bound(pts, v, f, face64, d64)
    print("%s: %d faces, max err %.3e, allowed %.3e .. %.3e" % (name, len(f), err.max(), tol.min(), tol.max()))
    assert (err <= tol).all()
    assert (face >= 0).all() and np.abs(np.linalg.norm(pts - q, axis=1) - d64).max() <= tol.max()


# ---------------------------------------------------------------------------------------------------------------------
# 5. sample_surface on CPU tensors
# ---------------------------------------------------------------------------------------------------------------------
def test_sample_surface_on_cpu():
    from connecting_the_dots_amd import mesheval
    v, f = bvh_scenes.icosphere(1)
    verts, faces = torch.from_numpy(v.astype(F)), torch.from_numpy(f.astype(np.int32))
    g = torch.Generator()
    g.manual_seed(5)
    p1, f1 = mesheval.sample_surface(verts, faces, 2000, generator=g)
    g.manual_seed(5)
    p2, f2 = mesheval.sample_surface(verts, faces, 2000, generator=g)
    assert torch.equal(p1, p2) and torch.equal(f1, f2) and p1.shape == (2000, 3) and p1.dtype == torch.float32
    assert f1.shape == (2000,) and int(f1.min()) >= 0 and int(f1.max()) < len(f) and len(f1.unique()) == len(f)
    # every sample lies on its face: the restatement's distance to that very face is within the bound (2) / (3) plus the
    # rounding of the sample itself, 4u (|a| + |b| + |c|) for w0 a + w1 b + w2 c
    pts, fi = p1.numpy(), f1.numpy()
    a, b, c = (v.astype(F)[f[fi, i]] for i in range(3))
    d2, _ = pr.point_tri(pts, a, b, c)
    own = 4 * pr.U * (np.linalg.norm(a, axis=1) + np.linalg.norm(b, axis=1) + np.linalg.norm(c, axis=1))
    tol = pr.forward_bound(pts, v.astype(F), f, fi, np.zeros(len(pts))) + own
    assert (np.sqrt(d2.astype(np.float64)) <= tol).all()
    assert mesheval.sample_surface(verts, faces, 0)[0].shape == (0, 3)
    # area weights: one face of 9 times the other's area takes 0.9 +- 4 sigma of 10 000 samples; zero-area and
    # non-finite faces get none
    verts = torch.tensor([[0, 0, 0], [3, 0, 0], [0, 3, 0], [10, 0, 0], [11, 0, 0], [10, 1, 0], [5, 5, 5], [6, 6, 6],
                          [float("nan"), 0, 0]], dtype=torch.float32)
    faces = torch.tensor([[6, 7, 6], [0, 1, 2], [6, 6, 6], [3, 4, 5], [0, 1, 8]], dtype=torch.int32)
    g.manual_seed(11)
    _, fi = mesheval.sample_surface(verts, faces, 10000, generator=g)
    share = float((fi == 1).float().mean())
    sigma = (0.9 * 0.1 / 10000) ** 0.5
    assert abs(share - 0.9) <= 4 * sigma and set(fi.unique().tolist()) == {1, 3}
    for bad in (dict(verts=verts.double()), dict(faces=faces.float()), dict(faces=faces[:, :2]), dict(n=-1), dict(n=2.0),
                dict(faces=faces[:0]), dict(faces=faces + 9), dict(faces=faces[[0, 2]])):
        with pytest.raises(RuntimeError):
            mesheval.sample_surface(**dict(dict(verts=verts, faces=faces, n=10), **bad))
