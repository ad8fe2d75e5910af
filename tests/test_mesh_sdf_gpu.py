"""GPU checks of the signed nearest-face query (ctd_point_mesh_signed_f32 of include/ctd_hip_mesh_sdf.h, csrc/mesh_sdf.hip;
connecting_the_dots_amd.meshsdf): both kernels bit for bit against the restatement tests/meshsdf_ref.py (d2, face,
closest and feature; the sign wherever the restatement's |dot| stands clear of the device atan2's rounding), the entry point
without a cutoff against ctd_point_mesh_distance_f32, the cutoff against the uncut answer, mesh_to_tsdf against the
point query it is made of, the way from a mesh to a volume and back, and the signed error of scaled spheres.

The sign condition.  The kernel's only operation that is not correctly rounded is the atan2 of the vertex weights, within
2 ulp (4.4e-16 relative), so its dot differs from the restatement's by at most about 4.4e-16 S with S = |r| * W; signs
must agree wherever |dot| > 1e-13 S (some 250 times that), both must be 0 where r == 0 or nothing contributes (S == 0:
these use no atan2), and elsewhere either answer passes -- for at most 0.1 % of a case's points, and on these fixtures
the restatement shows there is no such point at all."""
import functools

import numpy as np
import pytest
import torch

from tests import bvh_scenes
from tests import meshsdf_ref as sr
from tests import pointmesh_ref as pr
from tests import test_point_mesh_gpu as pm
from tests.test_point_mesh_gpu import DEV, F, OK, UNSUPPORTED, dev, dsqrt, same_bits

pytestmark = pytest.mark.gpu

INF = float("inf")
NAMES = ("d2", "face", "closest", "feature")


def rows_of(faces_t, n_verts):
    """the device's own adjacency of these faces -> the MeshAdjacency"""
    from connecting_the_dots_amd import meshsmooth
    return meshsmooth.MeshAdjacency(faces_t, n_verts)


def raw(points, verts, faces, adj, bvh=None, max_d2=INF, want_closest=True):
    """one call of the C entry point on device tensors -> (status, dict of numpy outputs); the outputs start as garbage
    the kernels have to overwrite"""
    from connecting_the_dots_amd import _lib
    n = points.shape[0]
    d2 = torch.full((n,), -7.0, dtype=torch.float32, device=DEV)
    face = torch.full((n,), -7, dtype=torch.int32, device=DEV)
    closest = torch.full((n, 3), -7.0, dtype=torch.float32, device=DEV) if want_closest else None
    feature = torch.full((n,), 77, dtype=torch.int8, device=DEV)
    sign = torch.full((n,), 77, dtype=torch.int8, device=DEV)
    ptr = lambda t: t.data_ptr() if t is not None and t.numel() else None     # noqa: E731
    st = _lib.lib().ctd_point_mesh_signed_f32(
        ptr(points), n, ptr(verts), verts.shape[0], ptr(faces), faces.shape[0], adj.face_offsets.data_ptr(),
        ptr(adj.face_ids) or adj.face_offsets.data_ptr(), adj.face_ids.shape[0],       # (no rows at all: any pointer but NULL)
        None if bvh is None else bvh.buffer.data_ptr(), max_d2, ptr(d2), ptr(face), ptr(closest), ptr(feature), ptr(sign),
        torch.cuda.current_device(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    out = dict(d2=d2.cpu().numpy(), face=face.cpu().numpy(), closest=None if closest is None else closest.cpu().numpy(),
               feature=feature.cpu().numpy(), sign=sign.cpu().numpy())
    return st, out


def assert_same(got, want, what, names=NAMES + ("sign",)):
    for name in names:
        g, w = got[name], want[name]
        if not same_bits(g, w):
            bad = np.where((g != w).reshape(len(g), -1).any(1) & ~(np.isnan(g) & np.isnan(w)).reshape(len(g), -1).all(1))[0]
            raise AssertionError("%s: %s differs at %d of %d points, first %s: %s vs %s" % (
                what, name, len(bad), len(g), bad[:5], g[bad[:3]], w[bad[:3]]))


def undecided(want, points):
    """the points whose sign the restatement leaves to either answer: something contributes, r != 0, and |dot| does not
    stand clear of 1e-13 S"""
    r0 = (np.ascontiguousarray(points, F) == want["closest"]).all(1)
    return (want["face"] >= 0) & ~r0 & (want["S"] > 0) & ~(np.abs(want["dot"]) > 1e-13 * want["S"])


def assert_against_restatement(got, want, points, what):
    n = len(got["face"])
    w = {k: v[:n] for k, v in want.items()}
    assert_same(got, w, what, NAMES)
    loose = undecided(w, points[:n])
    assert loose.sum() <= 1e-3 * n, "%s: %d of %d points under the allowance" % (what, loose.sum(), n)
    bad = np.where(~loose & (got["sign"] != w["sign"]))[0]
    assert len(bad) == 0, "%s: sign differs at %d of %d points, first %s: %s vs %s, dot %s, S %s" % (
        what, len(bad), n, bad[:5], got["sign"][bad[:5]], w["sign"][bad[:5]], w["dot"][bad[:5]], w["S"][bad[:5]])
    r0 = (np.ascontiguousarray(points[:n], F) == w["closest"]).all(1)
    assert (got["sign"][r0 | (w["face"] < 0)] == 0).all()


# ---------------------------------------------------------------------------------------------------------------------
# 8. both kernels against the restatement
# ---------------------------------------------------------------------------------------------------------------------
N_POINTS = (0, 1, 63, 64, 65, 257, 1000)


def around(verts, rs, n=1000, spread=0.6):
    """n points: near the vertices, then uniform in the bounding box grown by `spread`"""
    verts = np.asarray(verts, np.float64)
    near = verts[rs.randint(0, len(verts), n // 2)] + rs.normal(size=(n // 2, 3)) * 0.05
    lo, hi = verts.min(0) - spread, verts.max(0) + spread
    return np.concatenate([near, rs.uniform(lo, hi, size=(n - n // 2, 3))]).astype(F)


def on_the_mesh(verts, faces, rs, n):
    """points exactly on vertices, on edge midpoints and on face interiors, n of each (f32 arithmetic)"""
    verts, faces = np.asarray(verts, F), np.asarray(faces)
    a, b, c = (verts[faces[rs.randint(0, len(faces), n), k]] for k in range(3))
    return np.concatenate([verts[rs.randint(0, len(verts), n)], (a + b) / F(2), (a + b) / F(4) + c / F(2)]).astype(F)


def case(name):
    """-> (verts f32, faces int32, points f32 [1000,3], with_tree)"""
    rs = np.random.RandomState(sum(map(ord, name)))
    if name == "one face":
        v, f = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], F), np.array([[0, 1, 2]], np.int32)
        return v, f, around(v, rs, spread=1.0), True
    if name == "wedge":
        v, f = sr.wedge()
        return v, f, np.concatenate([sr.wedge_points(700, 5), on_the_mesh(v, f, rs, 100)]), True
    if name == "cube":
        v, f = sr.cube()
        return v, f, np.concatenate([rs.uniform(-2, 2, size=(700, 3)).astype(F), on_the_mesh(v, f, rs, 100)]), True
    if name == "grid":
        v, f = pm.grid_mesh(16)                                       # 512 faces, open: two brute-force tiles
        xy = rs.uniform(-0.5, 2.5, size=(1000, 2))                    # the grid spans [0, 2]^2: inside and beyond the rim
        z = np.where(rs.rand(1000) < 0.5, 1, -1) * rs.uniform(0.01, 0.7, size=1000)
        return v, f, np.concatenate([xy, z[:, None]], 1).astype(F), True
    if name == "soup257":
        v, f = pm.brute_mesh(257)                                     # out-of-range and repeated indices: brute force only
        return v, f, pm.brute_points(v, rs), False
    if name == "icosphere3":
        v, f = bvh_scenes.icosphere(3)
        v, f = v.astype(F), f.astype(np.int32)
        return v, f, np.concatenate([around(v, rs, 400, 0.3), on_the_mesh(v, f, rs, 200)]), True
    if name == "torus":
        v, f = bvh_scenes.torus(24, 12)
        v, f = v.astype(F), f.astype(np.int32)
        return v, f, np.concatenate([around(v, rs, 400, 0.3), on_the_mesh(v, f, rs, 200)]), True
    if name == "cone40":
        v, f = sr.cone(40)                                            # the apex has 40 incident faces
        above = np.array([0, 0, 1]) + rs.normal(size=(400, 3)) * [0.05, 0.05, 0.2]
        beside = np.array([0, 0, 0.9]) + rs.normal(size=(300, 3)) * [0.3, 0.3, 0.05]
        return v, f, np.concatenate([above, beside, around(v, rs, 300, 0.5)]).astype(F), True
    if name == "fan3":
        v, f = sr.fan3()                                              # three faces on one edge
        on_edge = np.stack([rs.uniform(0, 1, 300), rs.normal(size=300) * 0.1, rs.normal(size=300) * 0.1], 1)
        return v, f, np.concatenate([on_edge, around(v, rs, 700, 0.5)]).astype(F), True
    if name == "nonfinite points":
        v, f = sr.cube()
        pts = rs.uniform(-2, 2, size=(1000, 3)).astype(F)
        pts[::7, 0] = np.nan
        pts[3::7, 1] = np.inf
        pts[5::7, 2] = -np.inf
        pts[6::7] = 1e30                                              # d2 overflows: no face qualifies
        return v, f, pts, True
    raise KeyError(name)


CASES = ("one face", "wedge", "cube", "grid", "soup257", "icosphere3", "torus", "cone40", "fan3", "nonfinite points")


@pytest.mark.parametrize("name", CASES)
def test_kernels_against_the_restatement(name):
    from connecting_the_dots_amd import renderer
    verts, faces, pts, with_tree = case(name)
    assert len(pts) == N_POINTS[-1]
    want = sr.signed(pts, verts, faces)                               # once, for the 1000 points
    loose = undecided(want, pts)
    clear = (want["S"] > 0) & (want["d2"] > 0)
    print("%s: %d faces, features %s, signs %s, %d under the allowance, smallest |dot| / S %.3g" % (
        name, len(faces), np.bincount(want["feature"][want["face"] >= 0], minlength=7),
        np.bincount(want["sign"] + 1, minlength=3), loose.sum(), (np.abs(want["dot"][clear]) / want["S"][clear]).min()))
    assert loose.sum() == 0                                           # the restatement alone: it leaves out none
    v, f = dev(verts, F), dev(faces, np.int32)
    adj = rows_of(f, len(verts))
    fo, fi = sr.incident_rows(faces, len(verts))
    assert np.array_equal(adj.face_offsets.cpu().numpy(), fo) and np.array_equal(adj.face_ids.cpu().numpy(), fi)
    if name == "cone40":
        assert adj.max_incident == 40 and (want["feature"] == 2).sum() > 100      # the long row is walked
    bvh = renderer.MeshBVH(v, f) if with_tree else None
    for n in N_POINTS:
        p = dev(pts[:n], F)
        st, got = raw(p, v, f, adj)
        assert st == OK
        assert_against_restatement(got, want, pts, "%s, brute force, %d points" % (name, n))
        if bvh is not None and bvh.usable:
            st, tree = raw(p, v, f, adj, bvh)
            assert st == OK
            assert_same(tree, got, "%s, tree against brute force, %d points" % (name, n))
    st, got = raw(dev(pts, F), v, f, adj, want_closest=False)          # closest is optional: the sign does not need it
    assert st == OK and got["closest"] is None
    assert_against_restatement(dict(got, closest=want["closest"]), want, pts, "%s, without closest" % name)


def test_an_empty_mesh_and_broken_rows():
    v, f = sr.cube()
    pts = dev(np.random.RandomState(0).uniform(-2, 2, size=(100, 3)), F)
    vt, ft = dev(v, F), dev(f, np.int32)
    adj = rows_of(ft, len(v))
    st, got = raw(pts, vt, ft[:0], rows_of(ft[:0], len(v)))
    assert st == OK and (got["face"] == -1).all() and np.isposinf(got["d2"]).all() and np.isnan(got["closest"]).all()
    assert (got["feature"] == -1).all() and (got["sign"] == 0).all()
    # rows of any values: nothing outside the buffers is read, and what the rule does not accept adds nothing
    st, ref = raw(pts, vt, ft, adj)

    class Rows:
        pass

    for fo, fi in ((torch.full_like(adj.face_offsets, 1 << 30), adj.face_ids),
                   (-adj.face_offsets - 1, adj.face_ids),
                   (adj.face_offsets, torch.full_like(adj.face_ids, 1 << 30)),
                   (adj.face_offsets, -adj.face_ids - 1)):
        bad = Rows()
        bad.face_offsets, bad.face_ids = fo.contiguous(), fi.contiguous()
        st, got = raw(pts, vt, ft, bad)
        assert st == OK
        assert_same(got, ref, "broken rows", NAMES)
        inner = ref["feature"] == 6                                  # the interior needs no row
        assert np.array_equal(got["sign"][inner], ref["sign"][inner]) and (got["sign"][~inner] == 0).all()


# ---------------------------------------------------------------------------------------------------------------------
# 9. without a cutoff: ctd_point_mesh_distance_f32, bit for bit
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def scene_points():
    v, f = pm.scene2000()
    rs = np.random.RandomState(1)
    near = (v[6:] + rs.normal(size=v[6:].shape) * 1e-3).astype(F)
    far = (rs.normal(size=(1000, 3)) * 1e3).astype(F)
    box = rs.uniform(v[6:].min(0), v[6:].max(0), size=(2000, 3)).astype(F)
    return near, far, box


def mean_edge(v, f):
    V = v.astype(np.float64)
    a, b, c = (V[f[2:, k]] for k in range(3))                       # without the two faces of the 1000-unit board
    return float(np.mean([np.linalg.norm(b - a, axis=1).mean(), np.linalg.norm(c - b, axis=1).mean(),
                          np.linalg.norm(a - c, axis=1).mean()]))


def test_without_cutoff_it_is_point_mesh_distance():
    from connecting_the_dots_amd import renderer
    v, f = pm.scene2000()
    near, far, _ = scene_points()
    shifted = ((near[::3].astype(np.float64) + 1e3).astype(F), (v.astype(np.float64) + 1e3).astype(F))
    for what, pts, verts in (("near", near, v), ("far", far, v), ("translated by 1e3", shifted[0], shifted[1])):
        p, vt, ft = dev(pts, F), dev(verts, F), dev(f, np.int32)
        adj, bvh = rows_of(ft, len(verts)), renderer.MeshBVH(vt, ft)
        assert bvh.usable
        for tree in (None, bvh):
            st, *old = pm.raw(p, vt, ft, tree)
            st2, new = raw(p, vt, ft, adj, tree)
            assert st == st2 == OK
            pm.assert_same([new["d2"], new["face"], new["closest"]], old, "%s, tree %s" % (what, tree is not None))
            assert ((new["feature"] >= 0) == (new["face"] >= 0)).all()


# ---------------------------------------------------------------------------------------------------------------------
# 10. the cutoff
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("edges", [0.5, 2.0, 8.0])
def test_cutoff_is_the_uncut_answer_restricted(edges):
    from connecting_the_dots_amd import meshsdf, renderer
    v, f = pm.scene2000()
    near, far, box = scene_points()
    pts = np.concatenate([near[::2], box, far[:200]])                # (the far points qualify under none of the cutoffs)
    max_dist = edges * mean_edge(v, f)
    max_d2 = meshsdf._max_d2(max_dist, "test")
    assert max_d2 == float(F(max_dist) * F(max_dist))
    p, vt, ft = dev(pts, F), dev(v, F), dev(f, np.int32)
    adj, bvh = rows_of(ft, len(v)), renderer.MeshBVH(vt, ft)
    st, full = raw(p, vt, ft, adj)
    st1, brute = raw(p, vt, ft, adj, None, max_d2)
    st2, tree = raw(p, vt, ft, adj, bvh, max_d2)
    assert st == st1 == st2 == OK and bvh.usable
    assert_same(tree, brute, "cutoff %g edges: tree against brute force" % edges)
    inside = full["d2"] <= F(max_d2)
    print("cutoff %g mean edge lengths = %.4f: %d of %d points qualify" % (edges, max_dist, inside.sum(), len(pts)))
    assert 0 < inside.sum() < len(pts)
    assert np.array_equal(brute["face"] >= 0, inside)
    none = dict(d2=np.full(len(pts), np.inf, F), face=np.full(len(pts), -1, np.int32), closest=np.full((len(pts), 3), np.nan, F),
                feature=np.full(len(pts), -1, np.int8), sign=np.zeros(len(pts), np.int8))
    want = {k: np.where(inside.reshape((-1,) + (1,) * (full[k].ndim - 1)), full[k], none[k]) for k in full}
    assert_same(brute, want, "cutoff %g edges: against the uncut answer" % edges)


def test_cutoff_at_its_exact_boundary_on_the_device():
    from connecting_the_dots_amd import renderer
    tri, one = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], F), np.array([[0, 1, 2]], np.int32)
    h = F(0.375)
    lim = F(h * h)
    pts = np.array([[0.25, 0.25, h], [0.25, 0.25, -h]], F)
    p, vt, ft = dev(pts, F), dev(tri, F), dev(one, np.int32)
    adj, bvh = rows_of(ft, 3), renderer.MeshBVH(vt, ft)
    for tree in (None, bvh):
        st, got = raw(p, vt, ft, adj, tree, float(lim))
        assert st == OK and got["face"].tolist() == [0, 0] and (got["d2"] == lim).all() and got["feature"].tolist() == [6, 6]
        assert got["sign"].tolist() == [1, -1] and np.array_equal(got["closest"], np.array([[0.25, 0.25, 0]] * 2, F))
        st, got = raw(p, vt, ft, adj, tree, float(np.nextafter(lim, F(0))))
        assert st == OK and got["face"].tolist() == [-1, -1] and np.isposinf(got["d2"]).all() and np.isnan(got["closest"]).all()
        assert got["feature"].tolist() == [-1, -1] and got["sign"].tolist() == [0, 0]
        st, got = raw(dev(tri, F), vt, ft, adj, tree, 0.0)            # max_d2 = 0: the points on the mesh still qualify
        assert st == OK and got["face"].tolist() == [0, 0, 0] and got["sign"].tolist() == [0, 0, 0]


# ---------------------------------------------------------------------------------------------------------------------
# 11. two calls give identical bytes
# ---------------------------------------------------------------------------------------------------------------------
def test_two_calls_give_identical_bytes():
    from connecting_the_dots_amd import renderer
    v, f = pm.scene2000()
    pts = (v[6:] + np.random.RandomState(3).normal(size=v[6:].shape) * 1e-2).astype(F)
    p, vt, ft = dev(pts, F), dev(v, F), dev(f, np.int32)
    adj, bvh = rows_of(ft, len(v)), renderer.MeshBVH(vt, ft)
    for tree in (None, bvh):
        for max_d2 in (INF, 1e-4):
            (sa, a), (sb, b) = raw(p, vt, ft, adj, tree, max_d2), raw(p, vt, ft, adj, tree, max_d2)
            assert sa == sb == OK
            assert_same(a, b, "second call")


# ---------------------------------------------------------------------------------------------------------------------
# 12. mesh_to_tsdf is the point query on the voxel centres
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims,origin,voxel,trunc", [((70, 6, 5), (-1.75, -0.1, 0.85), 0.05, 0.2),
                                                    ((5, 4, 3), (-1.25, -0.75, -0.5), 0.5, 1.5)])
def test_mesh_to_tsdf_is_the_point_query_on_the_centres(dims, origin, voxel, trunc):
    from connecting_the_dots_amd import meshsdf
    v, f = sr.cube()
    vt, ft = dev(v, F), dev(f, np.int32)
    nx, ny, nz = dims
    o = np.array(origin, F)
    cx, cy, cz = (o[c] + F(voxel) * np.arange(n, dtype=F) for c, n in enumerate(dims))        # one product, one sum, in f32
    assert cx.dtype == F
    zz, yy, xx = np.meshgrid(cz, cy, cx, indexing="ij")
    centres = np.stack([xx, yy, zz], -1).reshape(-1, 3)                                      # x fastest
    ot = torch.from_numpy(o).to(DEV)
    tsdf, weight = meshsdf.mesh_to_tsdf(vt, ft, ot, voxel, dims, trunc)
    assert tsdf.shape == weight.shape == (1, nz, ny, nx) and tsdf.dtype == weight.dtype == torch.float32
    sdist, face, feature, sign = meshsdf.point_mesh_signed_distance(dev(centres, F), vt, ft, max_dist=trunc, return_feature=True)
    hit = face >= 0
    want = torch.where(hit, torch.minimum(torch.ones((), device=DEV), sdist / torch.tensor(trunc, dtype=torch.float32, device=DEV)),
                       torch.zeros((), device=DEV))
    assert torch.equal(tsdf.view(-1).view(torch.int32), want.view(torch.int32))
    assert torch.equal(weight.view(-1), hit.float())
    n_hit = int(hit.sum())
    print("mesh_to_tsdf %s: %d of %d voxels within trunc, tsdf %.3f .. %.3f" % (dims, n_hit, hit.numel(), float(tsdf.min()), float(tsdf.max())))
    assert 0 < n_hit < hit.numel() or dims == (5, 4, 3)
    assert float(tsdf.min()) < 0 < float(tsdf.max()) and float(tsdf.abs().max()) <= 1.0
    assert bool((tsdf[weight == 0] == 0).all()) and set(weight.unique().tolist()) <= {0.0, 1.0}
    # the restatement on the same centres: the same nearest faces and signs
    ref = sr.signed(centres, v, f, float(F(trunc) * F(trunc)))
    assert np.array_equal(ref["face"], face.cpu().numpy()) and np.array_equal(ref["sign"], sign.cpu().numpy())
    # `chunk` does not change a bit: one slice per slab, two, and a chunk below one slice
    for chunk in (nx * ny, 2 * nx * ny + 1, 1):
        t2, w2 = meshsdf.mesh_to_tsdf(vt, ft, ot, voxel, dims, trunc, chunk=chunk)
        assert torch.equal(t2.view(torch.int32), tsdf.view(torch.int32)) and torch.equal(w2, weight)
    for bad in (dict(origin=ot.view(1, 3)), dict(voxel=0.0), dict(trunc=-1.0), dict(dims=(nx, ny)), dict(dims=(nx, 0, nz)),
                dict(chunk=0), dict(origin=ot.double())):
        with pytest.raises(RuntimeError):
            meshsdf.mesh_to_tsdf(**dict(dict(verts=vt, faces=ft, origin=ot, voxel=voxel, dims=dims, trunc=trunc), **bad))


# ---------------------------------------------------------------------------------------------------------------------
# 13. from a mesh to a volume and back
# ---------------------------------------------------------------------------------------------------------------------
def test_round_trip_through_a_volume():
    from connecting_the_dots_amd import mesh, mesheval, meshsdf, meshsmooth
    v, f = pm.sphere3()
    v = (v.astype(np.float64) * 0.5).astype(F)
    vt, ft = dev(v, F), dev(f, np.int32)
    n, voxel = 48, 0.03
    origin = torch.full((3,), -0.5 * (n - 1) * voxel, dtype=torch.float32, device=DEV)
    tsdf, weight = meshsdf.mesh_to_tsdf(vt, ft, origin, voxel, (n, n, n), 4 * voxel)
    m = mesh.tsdf_mesh(tsdf, weight, origin.view(1, 3), voxel)
    verts, faces, _ = m.track(0)
    adj = meshsmooth.MeshAdjacency(faces, verts.shape[0])
    assert faces.shape[0] > 1000 and adj.closed and adj.euler == 2
    dist, _ = mesheval.point_mesh_distance(verts, vt, ft)
    # a bound, not a measurement: both ends of a crossing grid edge lie within a voxel of the surface, and so does the
    # vertex between them
    e = meshsdf.signed_error(verts, faces, vt, ft)
    print("round trip: %d vertices, %d faces, max distance %.5f (voxel %.3f), signed mean %.6f, median %.6f, share outside %.3f"
          % (verts.shape[0], faces.shape[0], float(dist.max()), voxel, e["mean"], e["median"], e["share_outside"]))
    assert float(dist.max()) <= voxel
    assert abs(e["mean"]) < voxel and e["n"] == verts.shape[0] and e["n_unmatched"] == 0


# ---------------------------------------------------------------------------------------------------------------------
# 14. signed_error of scaled spheres
# ---------------------------------------------------------------------------------------------------------------------
def test_signed_error_of_scaled_spheres():
    from connecting_the_dots_amd import meshsdf
    v, f = pm.sphere3()
    # the interval of tests/test_point_mesh_gpu.test_reconstruction_error_of_a_scaled_sphere: every distance between the
    # unit icosphere and its copy scaled by 1.01 (or, by the same argument with the roles exchanged and the factor
    # 0.99 / 1 in place of 1 / 1.01, by 0.99: the inner mesh is then 0.99 times the outer one) lies in
    # [0.01 cos(t), 0.01 + sagitta], t the largest angle between a face's normal and one of its corners
    a, b, c = (v.astype(np.float64)[f[:, k]] for k in range(3))
    nrm = np.cross(b - a, c - a)
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    cos_t = min((nrm * a).sum(1).min(), (nrm * b).sum(1).min(), (nrm * c).sum(1).min())
    lo, hi = 0.01 * cos_t, 0.01 + (1 - cos_t)
    vt, ft = dev(v, F), dev(f, np.int32)
    for scale, side in ((1.01, 1.0), (0.99, 0.0)):
        sv = (v.astype(np.float64) * scale).astype(F)
        d2_64, face64, _ = pr.nearest(sv, v, f, np.float64)
        slack = 4 * pr.U * 1.01 + pr.forward_bound(sv, v, f, face64, np.sqrt(d2_64)).max()
        for bvh in (None, "auto"):
            e = meshsdf.signed_error(dev(sv, F), ft, vt, ft, bvh=bvh)
            print("sphere scaled by %.2f: mean %.6f, median %.6f, share outside %.1f, allowed |mean| %.6f .. %.6f" % (
                scale, e["mean"], e["median"], e["share_outside"], lo - slack, hi + slack))
            assert e["share_outside"] == side and e["n"] == len(v) and e["n_undetermined"] == 0 and e["n_unmatched"] == 0
            sgn = 1 if side else -1
            assert lo - slack <= sgn * e["mean"] <= hi + slack and lo - slack <= sgn * e["median"] <= hi + slack
    g = torch.Generator(device=DEV)
    g.manual_seed(9)
    sv = dev((v.astype(np.float64) * 1.01).astype(F), F)
    e = meshsdf.signed_error(sv, ft, vt, ft, n_samples=5000, generator=g)
    g.manual_seed(9)
    assert e == meshsdf.signed_error(sv, ft, vt, ft, n_samples=5000, generator=g)
    assert e["share_outside"] == 1.0 and e["n"] == 5000 and 0 < e["mean"] <= hi + slack
    with pytest.raises(RuntimeError, match="None or 'auto'"):
        meshsdf.signed_error(sv, ft, vt, ft, bvh=3)


# ---------------------------------------------------------------------------------------------------------------------
# 15. the Python module
# ---------------------------------------------------------------------------------------------------------------------
def test_auto_none_and_an_explicit_tree_agree(monkeypatch):
    from connecting_the_dots_amd import meshsdf, meshsmooth, renderer
    v, f = pm.scene2000()
    pts = (v[6:] + np.random.RandomState(4).normal(size=v[6:].shape) * 1e-2).astype(F)[:1500]
    p, vt, ft = dev(pts, F), dev(v, F), dev(f, np.int32)
    want = sr.signed(pts, v, f)
    assert undecided(want, pts).sum() == 0
    built = []
    real = renderer.MeshBVH
    adj = meshsmooth.MeshAdjacency(ft, len(v))
    kw = dict(return_closest=True, return_feature=True)
    outs = [meshsdf.point_mesh_signed_distance(p, vt, ft, bvh=None, **kw)]
    outs.append(meshsdf.point_mesh_signed_distance(p, vt, ft, bvh=real(vt, ft), adjacency=adj, **kw))
    monkeypatch.setattr(renderer, "MeshBVH", lambda *a, **k: built.append(1) or real(*a, **k))     # counts 'auto' builds
    outs.append(meshsdf.point_mesh_signed_distance(p, vt, ft, bvh="auto", **kw))
    assert len(built) == (len(f) >= meshsdf.AUTO_BVH_MIN_FACES)
    monkeypatch.setattr(meshsdf, "AUTO_BVH_MIN_FACES", 1024)
    outs.append(meshsdf.point_mesh_signed_distance(p, vt, ft, bvh="auto", **kw))                  # above it: builds
    assert len(built) >= 1
    monkeypatch.undo()
    dist = dsqrt(want["d2"])
    for sdist, face, closest, feature, sign in outs:
        assert sdist.dtype == torch.float32 and face.dtype == torch.int32 and closest.shape == (len(pts), 3)
        assert feature.dtype == sign.dtype == torch.int8
        assert same_bits(face.cpu().numpy(), want["face"]) and same_bits(closest.cpu().numpy(), want["closest"])
        assert same_bits(feature.cpu().numpy(), want["feature"]) and same_bits(sign.cpu().numpy(), want["sign"])
        assert same_bits(sdist.cpu().numpy(), np.where(want["sign"] < 0, -dist, dist))
    # the return arity follows each flag
    assert len(meshsdf.point_mesh_signed_distance(p, vt, ft)) == 2
    assert len(meshsdf.point_mesh_signed_distance(p, vt, ft, return_closest=True)) == 3
    assert len(meshsdf.point_mesh_signed_distance(p, vt, ft, return_feature=True)) == 4
    # a cutoff: +inf where no face qualifies
    sdist, face = meshsdf.point_mesh_signed_distance(p, vt, ft, max_dist=5e-3, bvh="auto")
    cut = want["d2"] <= F(5e-3) * F(5e-3)
    assert 0 < cut.sum() < len(pts) and np.array_equal(face.cpu().numpy() >= 0, cut)
    assert np.isposinf(sdist.cpu().numpy()[~cut]).all() and same_bits(sdist.cpu().numpy()[cut], np.where(want["sign"] < 0, -dist, dist)[cut])
    with pytest.raises(RuntimeError, match="other verts / faces"):
        meshsdf.point_mesh_signed_distance(p, vt, ft, bvh=real(vt.clone(), ft))
    with pytest.raises(RuntimeError, match="adjacency was built for other faces"):
        meshsdf.point_mesh_signed_distance(p, vt, ft, adjacency=meshsmooth.MeshAdjacency(ft.clone(), len(v)))
    with pytest.raises(RuntimeError, match="adjacency was built for other faces"):
        meshsdf.point_mesh_signed_distance(p, vt[:-1], ft[:2], adjacency=adj)
    with pytest.raises(RuntimeError, match="adjacency must be a MeshAdjacency"):
        meshsdf.point_mesh_signed_distance(p, vt, ft, adjacency=(adj.face_offsets, adj.face_ids))
    with pytest.raises(RuntimeError, match="unsupported dtype"):
        meshsdf.point_mesh_signed_distance(p.double(), vt, ft)
    with pytest.raises(RuntimeError, match="unsupported dtype"):
        meshsdf.point_mesh_signed_distance(p, vt, ft.long())
    with pytest.raises(RuntimeError, match=r"shaped \[n,3\]"):
        meshsdf.point_mesh_signed_distance(p.reshape(-1), vt, ft)
    with pytest.raises(RuntimeError, match="contiguous"):
        meshsdf.point_mesh_signed_distance(p[:, [2, 1, 0]].t().contiguous().t(), vt, ft)
    with pytest.raises(RuntimeError, match="True or False"):
        meshsdf.point_mesh_signed_distance(p, vt, ft, return_feature=1)
    with pytest.raises(RuntimeError, match="max_dist must be a finite number >= 0"):
        meshsdf.point_mesh_signed_distance(p, vt, ft, max_dist=-1.0)
    empty = meshsdf.point_mesh_signed_distance(p[:0], vt, ft, **kw)
    assert [tuple(t.shape) for t in empty] == [(0,), (0,), (0, 3), (0,), (0,)]
    none = meshsdf.point_mesh_signed_distance(p[:5], vt, ft[:0], **kw)            # no faces: nothing qualifies
    assert np.isposinf(none[0].cpu().numpy()).all() and (none[1] == -1).all() and (none[4] == 0).all()
