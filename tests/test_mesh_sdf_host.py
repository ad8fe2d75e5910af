"""CPU-only checks of the signed nearest-face query (include/ctd_hip_mesh_sdf.h: ctd_point_mesh_signed_f32;
connecting_the_dots_amd.meshsdf): the rule's sentences (header against ctypes table: tests/test_abi_and_host.py), argument
validation before any HIP call, the restatement tests/meshsdf_ref.py against tests/pointmesh_ref.py (bit for bit without a cutoff), and its
signs against geometry on four outward-oriented fixtures: a cube (the analytic box distance), a thin wedge (half-spaces; the
fixture on which the nearest face's own normal is wrong for more than a quarter of the points), an icosphere and a torus.

Measured with the restatement (numpy; the kernels have to give these bits, tests/test_mesh_sdf_gpu.py):
  cube, 4000 points:    0 sign mismatches; smallest |dot| / S 0.37
  wedge, 4000 points:   0 mismatches among the points farther than 1e-6 from every plane; the nearest face's normal alone
                        gets 1683 wrong; smallest |dot| / S 0.006
  icosphere(2), 3000:   0 mismatches outside the shell between the inscribed radius and 1; smallest |dot| / S 0.97
  torus(24, 12), 3000:  0 mismatches outside the faceting's margin"""
import os

import numpy as np
import pytest
import torch

from tests import bvh_scenes
from tests import meshsdf_ref as sr
from tests import pointmesh_ref as pr
from tests.test_point_mesh_gpu import brute_mesh, brute_points
from tests.test_tsdf_host import _Bufs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SDF_HEADER = os.path.join(ROOT, "include", "ctd_hip_mesh_sdf.h")
OK, INVALID_ARG = 0, 1
F = np.float32
INF = float("inf")


@pytest.fixture(scope="module")
def L():
    from connecting_the_dots_amd import _lib
    return _lib.lib()


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    if a.dtype.kind == "f":
        u = {4: np.uint32, 8: np.uint64}[a.dtype.itemsize]
        return bool(((a.view(u) == b.view(u)) | (np.isnan(a) & np.isnan(b))).all())
    return bool(np.array_equal(a, b))


# ---------------------------------------------------------------------------------------------------------------------
# 1. the header (header == ctypes table == exports: tests/test_abi_and_host.py, for every header)
# ---------------------------------------------------------------------------------------------------------------------
def test_the_header_states_the_rule():
    text = " ".join(open(SDF_HEADER).read().replace("*", " ").split())
    for phrase in ("Exactly the rule of ctd_hip_mesh_dist.h: the same point_tri, the same selection, the same skipped faces",
                   "A face qualifies when its d2 compares <= max_d2 and < +inf",
                   "With max_d2 = +inf the outputs d2, face and closest are those of ctd_point_mesh_distance_f32, bit for bit",
                   "If no face qualifies: face = -1, d2 = +inf, closest = NaN, feature = -1, sign = 0",
                   "a node is pruned when its bound exceeds min(best d2, max_d2)",
                   "The branch that point_tri took for the winning face, not a reclassification of the clamped parameters",
                   "0, 1, 2 for vertex a, b, c; 3, 4, 5 for edge ab, ac, bc; 6 for the interior",
                   "All of it in f64, computed from the f32 vertices",
                   "unit = c / l (three divisions) when l > 0 and l is finite",
                   "Interior of face f: N = c of f, not normalised",
                   "a boundary edge gets one term, a non-manifold edge all of its terms, i == j none",
                   "alpha_g = atan2(sqrt((xx xx + xy xy) + xz xz), (u0 w0 + u1 w1) + u2 w2)",
                   "dot = (r0 N0 + r1 N1) + r2 N2",
                   "A row is empty unless 0 <= face_offsets[i] <= face_offsets[i+1] <= n_incident",
                   "A face id outside [0, n_faces) is never dereferenced",
                   "A vertex index outside [0, n_verts) is never dereferenced",
                   "for a max_d2 that is NaN or negative",
                   "CTD_ERR_UNSUPPORTED for a tree deeper than the traversal stack"):
        assert phrase in text, phrase


# ---------------------------------------------------------------------------------------------------------------------
# 2. validation before any HIP call
# ---------------------------------------------------------------------------------------------------------------------
def test_rejections_need_no_gpu(L):
    bufs = _Bufs(["points", "verts", "faces", "fo", "fi", "bvh", "d2", "face", "closest", "feature", "sign"])

    def call(n=10, nv=10, nf=10, ni=30, max_d2=INF, **ptrs):
        p = dict(bufs.ptr, **ptrs)
        return L.ctd_point_mesh_signed_f32(p["points"], n, p["verts"], nv, p["faces"], nf, p["fo"], p["fi"], ni, p["bvh"], max_d2,
                                           p["d2"], p["face"], p["closest"], p["feature"], p["sign"], -1, None)

    for kw in (dict(n=-1), dict(nv=-1), dict(nf=-1), dict(ni=-1), dict(ni=-(1 << 40)), dict(n=(1 << 31) // 3 + 1),
               dict(nf=(1 << 28) + 1), dict(max_d2=float("nan")), dict(max_d2=-1e-30), dict(max_d2=-INF), dict(points=None),
               dict(d2=None), dict(face=None), dict(feature=None), dict(sign=None), dict(fo=None), dict(fi=None),
               dict(verts=None), dict(faces=None), dict(bvh=bufs.ptr["bvh"] + 4), dict(bvh=bufs.ptr["bvh"] + 8),
               dict(n=-1, bvh=None), dict(faces=None, bvh=None), dict(n=0, nf=-1), dict(n=0, ni=-1), dict(n=0, max_d2=-1.0),
               dict(n=0, max_d2=float("nan")), dict(n=0, bvh=bufs.ptr["bvh"] + 4)):
        assert call(**kw) == INVALID_ARG, kw
    # nothing to do: CTD_OK before any HIP call, with or without a tree, the optional and the unused pointers NULL or not
    assert call(n=0) == OK and call(n=0, bvh=None, closest=None, max_d2=0.0) == OK
    assert call(n=0, points=None, d2=None, face=None, feature=None, sign=None, fo=None, fi=None, nf=0, verts=None, faces=None,
                ni=0) == OK


def test_meshsdf_rejections_need_no_gpu():
    from connecting_the_dots_amd import meshsdf
    assert sorted(n for n in vars(meshsdf) if not n.startswith("_") and
                  getattr(getattr(meshsdf, n), "__module__", "") == meshsdf.__name__) == [
        "mesh_to_tsdf", "point_mesh_signed_distance", "signed_error"]
    p, v = torch.zeros(4, 3), torch.zeros(5, 3)
    f = torch.zeros(2, 3, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="CUDA tensor"):
        meshsdf.point_mesh_signed_distance(p, v, f)
    with pytest.raises(RuntimeError, match="CUDA tensor"):
        meshsdf.mesh_to_tsdf(v, f, torch.zeros(3), 0.1, (4, 4, 4), 0.3)
    with pytest.raises(RuntimeError, match="CUDA tensor"):
        meshsdf.signed_error(v, f, v, f)
    with pytest.raises(RuntimeError, match="must be a tensor"):
        meshsdf.point_mesh_signed_distance(p.numpy(), v, f)
    t = meshsdf.AUTO_BVH_MIN_FACES
    assert t >= 2 and t & (t - 1) == 0
    # the cutoff: one f32 product; None is no cutoff
    assert meshsdf._max_d2(None, "w") == INF
    assert meshsdf._max_d2(0.1, "w") == float(F(0.1) * F(0.1)) and meshsdf._max_d2(0, "w") == 0.0
    assert meshsdf._max_d2(1e30, "w") == INF                                            # overflows: no cutoff
    for bad in (-1.0, float("nan"), INF, "1", True):
        with pytest.raises(RuntimeError, match="max_dist must be a finite number >= 0"):
            meshsdf._max_d2(bad, "w")


# ---------------------------------------------------------------------------------------------------------------------
# 3. without a cutoff the restatement is pointmesh_ref's, bit for bit
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mesh", ["soup257", "icosphere"])
def test_restatement_without_cutoff_is_pointmesh_ref(mesh):
    if mesh == "soup257":
        verts, faces = brute_mesh(257)                                 # with three faces whose indices are out of range
        pts = brute_points(verts, np.random.RandomState(257))[::2]
    else:
        v, f = bvh_scenes.icosphere(2)
        verts, faces = v.astype(F), f.astype(np.int32)
        pts = np.concatenate([np.random.RandomState(3).uniform(-1.5, 1.5, size=(400, 3)), verts[::3]]).astype(F)
    want = pr.nearest(pts, verts, faces)
    d2, face, closest, feature = sr.nearest(pts, verts, faces, np.inf)
    assert same_bits(d2, want[0]) and same_bits(face, want[1]) and same_bits(closest, want[2])
    assert feature.dtype == np.int8 and ((feature >= 0) == (face >= 0)).all() and feature.max() <= 6
    # a vertex region returns the vertex itself
    Fa = np.asarray(faces)
    for k in (0, 1, 2):
        sel = feature == k
        assert same_bits(closest[sel], verts[Fa[face[sel], k]])


# ---------------------------------------------------------------------------------------------------------------------
# 4. signs against geometry
# ---------------------------------------------------------------------------------------------------------------------
def test_cube_signs_are_the_box_distance_signs():
    v, f = sr.cube()
    pts = np.random.RandomState(0).uniform(-2, 2, size=(4000, 3)).astype(F)
    out = sr.signed(pts, v, f)
    truth = sr.box_sdf(pts)
    assert (truth != 0).all()
    assert np.array_equal(out["sign"], np.sign(truth).astype(np.int8))
    d2_64, face64, _ = pr.nearest(pts, v, f, np.float64)
    tol = pr.forward_bound(pts, v, f, face64, np.sqrt(d2_64))
    err = np.abs(np.sqrt(out["d2"].astype(np.float64)) - np.abs(truth))
    print("cube: max | |sdist| - |box distance| | %.3e, allowed %.3e .. %.3e; smallest |dot| / S %.3f; features %s" % (
        err.max(), tol.min(), tol.max(), (np.abs(out["dot"]) / out["S"]).min(), np.bincount(out["feature"], minlength=7)))
    assert (err <= tol).all()
    assert (np.bincount(out["feature"], minlength=7)[[3, 4, 5, 6]] > 0).all() and (out["feature"] < 3).sum() > 100


def test_wedge_needs_the_pseudonormal():
    v, f = sr.wedge()
    pts = sr.wedge_points()
    out = sr.signed(pts, v, f)
    pd = sr.plane_distances(pts, v, f).max(1)                       # convex: inside iff behind every face's plane
    clear = np.abs(pd) > 1e-6
    truth = np.where(pd > 0, 1, -1).astype(np.int8)
    wrong = int((out["sign"][clear] != truth[clear]).sum())
    # the nearest face's own normal: what an unsigned query plus one face normal would answer
    V = v.astype(np.float64)
    a, b, c = (V[f[out["face"], k]] for k in range(3))
    naive = np.sign(((pts.astype(np.float64) - out["closest"].astype(np.float64)) * np.cross(b - a, c - a)).sum(1)).astype(np.int8)
    naive_wrong = int((naive[clear] != truth[clear]).sum())
    print("wedge: %d of %d points clear of the planes, %d wrong signs, %d with the nearest face's normal; smallest |dot| / S "
          "%.3f; inside %d" % (clear.sum(), len(pts), wrong, naive_wrong, (np.abs(out["dot"]) / out["S"])[clear].min(),
                               (truth < 0).sum()))
    assert clear.sum() > 3990 and wrong == 0
    assert naive_wrong > 1000
    assert (truth < 0).sum() > 20                                   # some points do lie inside the sliver


def test_icosphere_signs():
    v, f = bvh_scenes.icosphere(2)
    v, f = v.astype(F), f.astype(np.int32)
    rs = np.random.RandomState(2)
    d = rs.normal(size=(3000, 3))
    pts = (d / np.linalg.norm(d, axis=1, keepdims=True) * rs.uniform(0.2, 1.8, size=(3000, 1))).astype(F)
    out = sr.signed(pts, v, f)
    V = v.astype(np.float64)
    a, b, c = (V[f[:, k]] for k in range(3))
    nrm = np.cross(b - a, c - a)
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    inscribed = (nrm * a).sum(1).min()
    rad = np.linalg.norm(pts.astype(np.float64), axis=1)
    inside, outside = rad < inscribed - 1e-3, rad > 1 + 1e-3
    print("icosphere(2): inscribed radius %.5f, %d inside, %d outside of 3000; smallest |dot| / S %.3f" % (
        inscribed, inside.sum(), outside.sum(), (np.abs(out["dot"]) / out["S"]).min()))
    assert inside.sum() > 1000 and outside.sum() > 1000 and inside.sum() + outside.sum() > 2900
    assert (out["sign"][inside] == -1).all() and (out["sign"][outside] == 1).all()


def test_torus_signs():
    R, r = 0.7, 0.3
    v, f = bvh_scenes.torus(24, 12, R, r)
    v, f = v.astype(F), f.astype(np.int32)

    def torus_sdf(p):
        p = np.asarray(p, np.float64)
        return np.hypot(np.hypot(p[..., 0], p[..., 1]) - R, p[..., 2]) - r

    # the faceting's sagitta: the vertices lie on the torus, a flat face leaves it most at its edges' midpoints and its
    # centroid; twice the largest of these as the margin
    V = v.astype(np.float64)
    a, b, c = (V[f[:, k]] for k in range(3))
    probes = np.concatenate([(a + b) / 2, (b + c) / 2, (a + c) / 2, (a + b + c) / 3])
    margin = 2 * np.abs(torus_sdf(probes)).max()
    pts = np.random.RandomState(4).uniform([-1.3, -1.3, -0.6], [1.3, 1.3, 0.6], size=(3000, 3)).astype(F)
    out = sr.signed(pts, v, f)
    truth = torus_sdf(pts)
    inside, outside = truth < -margin, truth > margin
    print("torus(24, 12): margin %.4f, %d inside, %d outside of 3000" % (margin, inside.sum(), outside.sum()))
    assert margin < 0.05 and inside.sum() > 150 and outside.sum() > 1500
    assert (out["sign"][inside] == -1).all() and (out["sign"][outside] == 1).all()


# ---------------------------------------------------------------------------------------------------------------------
# 5. - 7. features, edges and the cutoff by hand
# ---------------------------------------------------------------------------------------------------------------------
TRI = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], F)
ONE = np.array([[0, 1, 2]], np.int32)


def test_one_point_in_each_of_the_seven_regions():
    pts = np.array([[-1, -1, 0.5], [2, -0.5, 0], [-0.5, 2, 0], [0.5, -1, 0], [-1, 0.5, 0], [1, 1, 0], [0.25, 0.25, 2]], F)
    d2, face, q, feature = sr.nearest(pts, TRI, ONE)
    assert feature.tolist() == [0, 1, 2, 3, 4, 5, 6] and (face == 0).all()
    assert np.array_equal(d2, np.array([2.25, 1.25, 1.25, 1.0, 1.0, 0.5, 4.0], F))
    # the same regions whichever corner is stored first: the code names the stored corner or edge
    d2, face, q, feature = sr.nearest(pts, TRI, np.array([[1, 2, 0]]))
    assert feature.tolist() == [2, 0, 1, 4, 5, 3, 6]


def test_edges_boundary_three_faces_and_a_repeated_index():
    # a boundary edge of a single triangle takes that face's normal
    pts = np.array([[0.5, -1, 0.5], [0.5, -1, -0.5], [0.5, -1, 0], [-1, -1, 0.25], [-1, -1, -0.25]], F)
    out = sr.signed(pts, TRI, ONE)
    assert out["feature"].tolist() == [3, 3, 3, 0, 0] and out["sign"].tolist() == [1, -1, 0, 1, -1]
    rows = sr.incident_rows(ONE, 3)
    N, W = sr.pseudonormal(TRI, ONE.tolist(), *rows, 0, 3)
    assert N == [0.0, 0.0, 1.0] and W == 1.0
    N, W = sr.pseudonormal(TRI, ONE.tolist(), *rows, 0, 0)          # the right angle at a: alpha = pi / 2
    assert N == [0.0, 0.0, np.pi / 2] and W == np.pi / 2
    # an edge shared by three faces sums three unit normals, in face order
    v, f = sr.fan3()
    rows = sr.incident_rows(f, len(v))
    N, W = sr.pseudonormal(v, f.tolist(), *rows, 0, 3)
    units = [sr._unit(v, g) for g in f.tolist()]
    want = [(units[0][k] + units[1][k]) + units[2][k] for k in range(3)]
    assert W == 3.0 and N == want
    for g, code in ((1, 3), (2, 3)):                                # from every face on it, whatever its winding
        assert sr.pseudonormal(v, f.tolist(), *rows, g, code) == (want, 3.0)
    # a face with a repeated index: it can win (a degenerate face is an ordinary face for the distance) but it is not a
    # valid face, so nothing contributes and the sign is 0 in every region
    deg = np.array([[0, 1, 1], [2, 2, 2], [0, 2, 0]], np.int32)
    out = sr.signed(np.array([[0.5, -1, 0.5], [-1, -1, 0.5], [2, 0.5, 1], [0.2, 0.9, -1]], F), TRI, deg)
    assert (out["face"] >= 0).all() and (out["sign"] == 0).all() and (out["d2"] > 0).all()
    # rows are any values: broken offsets make the row empty, foreign ids are skipped
    fo, fi = sr.incident_rows(ONE, 3)
    for bad_rows in ((np.array([0, 5, 2, 3], np.int32), fi), (np.array([-1, 1, 2, 3], np.int32), fi),
                     (fo, np.array([7, -1, 5], np.int32))):
        out = sr.signed(pts[:2], TRI, ONE, rows=bad_rows)
        assert out["sign"].tolist() == [0, 0]


def test_the_cutoff_at_its_exact_boundary():
    h = F(0.375)
    p = np.array([[0.25, 0.25, h]], F)
    lim = F(h * h)
    d2, face, q, feature = sr.nearest(p, TRI, ONE, lim)
    assert d2[0] == lim and face[0] == 0 and feature[0] == 6 and np.array_equal(q[0], np.array([0.25, 0.25, 0], F))
    out = sr.signed(p, TRI, ONE, np.nextafter(lim, F(0)))
    assert out["face"][0] == -1 and np.isposinf(out["d2"][0]) and np.isnan(out["closest"]).all()
    assert out["feature"][0] == -1 and out["sign"][0] == 0
    assert sr.signed(p, TRI, ONE, lim)["sign"][0] == 1 and sr.signed(p * [1, 1, -1], TRI, ONE, lim)["sign"][0] == -1
    assert sr.nearest(p, TRI, ONE, 0.0)[1][0] == -1 and sr.nearest(TRI, TRI, ONE, 0.0)[1].tolist() == [0, 0, 0]
