"""GPU parity of the point-cloud family (pointcloud.PointGrid, knn, neighbor_mean_distance, statistical_outlier_mask,
estimate_normals, voxel_downsample; include/ext/ctd_hip_point_cloud.h) against tests/pointcloud_ref.py.

`knn` equals the brute-force restatement bit for bit, idx and d2, for every cell size: the default, one so small that
almost every occupied cell holds a single point, and one so large that all points share a cell.  The shapes are the
smallest at which each mechanism can go wrong: fewer points than k, more than one wavefront, a grid of one cell, rings that
run to the end of the grid, points on cell boundaries, a far point, points that are not finite.  mean_dist, the covariance
rows and the voxel means are bit-equal too (f64 sums in the stated order); the normal is held to 1e-6 rad of numpy's eigh
where the restatement's relative eigenvalue gap is at least 1e-3: the f64 eigenvector error at that gap is of the order
1e-12, rounding a unit vector to f32 moves it by at most about 1.2e-7 rad, and 1e-6 leaves a factor 8."""
import numpy as np
import pytest
import torch

from tests import fusion_ref as fr
from tests import meshreg_ref as mr
from tests import pointcloud_ref as pr
from tests.test_mesh_register_host import MAX_ROT_DEG, MAX_T

pytestmark = pytest.mark.gpu

F = np.float32
KS = (1, 8, 16, 33, 64)
HUGE = 64.0                                            # a cell that holds every point of the unit cube, and the far point
TINY = {1: 0.1, 2: 0.1, 63: 0.08, 65: 0.08, 257: 0.05, 1500: 0.03}    # the unit cube has far more such cells than points
MAX_NORMAL_RAD = 1e-6
MIN_GAP = 1e-3


@pytest.fixture(scope="module")
def pc():
    from connecting_the_dots_amd import pointcloud
    return pointcloud


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.cpu().numpy()


def cloud(n, seed=0):
    return np.random.RandomState(seed).rand(n, 3).astype(F)


def same_lists(got, want, what):
    (gi, gd), (wi, wd) = got, want
    gi, gd = host(gi), host(gd)
    assert gi.dtype == np.int32 and gd.dtype == F and gi.shape == wi.shape and gd.shape == wd.shape, what
    assert np.array_equal(gd.view(np.int32), wd.view(np.int32)), "%s: %d d2 values differ" % (what, int((gd != wd).sum()))
    assert np.array_equal(gi, wi), "%s: %d indices differ" % (what, int((gi != wi).sum()))


_FULL = {}


def reference(n, max_dist, seed=0):
    """the restatement at k = 64, once per case and shared: a shorter list is its prefix (the order is total)"""
    key = (n, max_dist, seed)
    if key not in _FULL:
        _FULL[key] = pr.knn(cloud(n, seed), 64, max_dist=max_dist)
    return _FULL[key]


@pytest.mark.parametrize("n", [1, 2, 63, 65, 257, 1500])
def test_knn_equals_the_restatement(pc, n):
    pts = dev(cloud(n))
    before = pts.clone()
    for cell in (None, TINY[n], HUGE):
        grid = pc.PointGrid(pts, cell)
        assert grid.n_finite == n and grid.order.dtype == torch.int32 and int(grid.start[-1]) == n
        assert sorted(host(grid.order).tolist()) == list(range(n)) and (np.diff(host(grid.keys)) > 0).all()
        assert grid.nbytes > 0
        if cell == HUGE:
            assert grid.n_cells == 1 and grid.dims == (1, 1, 1)
        if cell == TINY[n]:
            assert grid.n_cells >= 0.9 * n                          # almost every occupied cell holds one point
        for max_dist in (None, 0.07, 5.0):
            wi, wd = reference(n, max_dist)
            for k in KS:
                same_lists(pc.knn(grid, k, max_dist=max_dist), (wi[:, :k], wd[:, :k]),
                           "n %d, k %d, cell %r, max_dist %r" % (n, k, cell, max_dist))
    assert torch.equal(pts, before)


@pytest.mark.parametrize("q", [1, 65, 300])
def test_knn_of_separate_queries(pc, q):
    rs = np.random.RandomState(q)
    pts = cloud(257)
    queries = rs.uniform(-0.6, 1.6, (q, 3)).astype(F)              # many of them outside the box of the points
    queries[::7] = pts[rs.randint(0, len(pts), len(queries[::7]))]  # some on a point: d2 = 0 and nothing is excluded
    if q > 2:
        queries[1], queries[2] = (np.nan, 0, 0), (0, np.inf, 0)
    for cell in (None, TINY[257], HUGE):
        grid = pc.PointGrid(dev(pts), cell)
        for max_dist in (None, 0.2):
            for k in (1, 16, 64):
                want = pr.knn(pts, k, queries=queries, max_dist=max_dist)
                same_lists(pc.knn(grid, k, queries=dev(queries), max_dist=max_dist), want, "q %d k %d cell %r" % (q, k, cell))
    if q > 2:
        idx, d2 = pc.knn(grid, 4, queries=dev(queries))
        assert (host(idx)[1:3] == -1).all() and np.isinf(host(d2)[1:3]).all() and (host(idx)[0] >= 0).all()
    assert pc.knn(grid, 4, queries=dev(queries[:0]))[0].shape == (0, 4)


def test_points_on_cell_boundaries(pc):
    """an exact lattice of spacing 0.3 with a cell of 0.3, not a power of two: every point sits on a cell boundary, the f32
    quotient decides its side, and most neighbours are equidistant"""
    i = np.arange(8, dtype=F)
    pts = np.stack(np.meshgrid(i, i, i, indexing="ij"), -1).reshape(-1, 3) * F(0.3) + F(0.1)
    pts = np.ascontiguousarray(pts[np.random.RandomState(0).permutation(len(pts))], F)
    for cell in (0.3, None, 0.1, HUGE):
        grid = pc.PointGrid(dev(pts), cell)
        for k in (6, 26, 64):
            same_lists(pc.knn(grid, k), pr.knn(pts, k), "lattice, k %d, cell %r" % (k, cell))
        same_lists(pc.knn(grid, 26, max_dist=0.3), pr.knn(pts, 26, max_dist=0.3), "lattice with max_dist, cell %r" % (cell,))


def test_one_far_point(pc):
    """1500 points of the unit cube and one at (4, 4, 4): its search walks the empty grid up to the others.  Never a
    statement about time."""
    pts = np.concatenate([cloud(1500), [[4, 4, 4]]]).astype(F)
    want = pr.knn(pts, 16)
    assert want[0][1500, 0] >= 0 and not (want[0][:1500] == 1500).any()
    for cell in (None, TINY[1500], HUGE):
        grid = pc.PointGrid(dev(pts), cell)
        free = pc.knn(grid, 16)
        same_lists(free, want, "far point, cell %r" % (cell,))
        capped = pc.knn(grid, 16, max_dist=8.0)                        # reaches everything: the same lists
        assert torch.equal(capped[0], free[0]) and torch.equal(capped[1].view(torch.int32), free[1].view(torch.int32))
        same_lists(pc.knn(grid, 16, max_dist=0.5), pr.knn(pts, 16, max_dist=0.5), "far point cut off, cell %r" % (cell,))


def test_the_order_of_the_points_does_not_matter(pc):
    rs = np.random.RandomState(3)
    pts = cloud(1500, 3)
    pts[1000:1100] = pts[:100]                                          # coincident pairs: ties in every list they enter
    perm = rs.permutation(len(pts))
    k = 16
    i0, d0 = (host(x) for x in pc.knn(pc.PointGrid(dev(pts)), k + 1))
    i1, d1 = (host(x) for x in pc.knn(pc.PointGrid(dev(pts[perm])), k + 1))
    back = np.empty_like(perm)
    back[perm] = np.arange(len(perm))                                   # pts[perm][j] is pts[perm[j]]: row back[i] is point i's
    i1, d1 = perm[i1[back]], d1[back]
    assert np.array_equal(d0.view(np.int32), d1.view(np.int32))
    tied = (np.diff(d0, axis=1) == 0).any(1)                            # (the k+1-th entry guards the end of the list)
    assert tied.any() and not tied.all()
    assert np.array_equal(i0[~tied, :k], i1[~tied, :k])
    inner = tied & (d0[:, k - 1] != d0[:, k])                           # tied, but not across the end of the list
    assert inner.any() and all(set(a) == set(b) for a, b in zip(i0[inner, :k], i1[inner, :k]))


def test_points_that_are_not_finite(pc):
    pts = cloud(1500, 5)
    rs = np.random.RandomState(5)
    bad = rs.choice(1500, 40, replace=False)
    pts[bad[:15], rs.randint(0, 3, 15)] = np.nan
    pts[bad[15:28], rs.randint(0, 3, 13)] = np.inf
    pts[bad[28:], rs.randint(0, 3, 12)] = -np.inf
    for cell in (None, TINY[1500], HUGE):
        grid = pc.PointGrid(dev(pts), cell)
        assert grid.n_finite == 1460 and grid.sorted_points.shape == (1460, 3)
        assert sorted(host(grid.order)[1460:].tolist()) == sorted(bad.tolist())
        idx, d2 = pc.knn(grid, 16)
        same_lists((idx, d2), pr.knn(pts, 16), "non-finite points, cell %r" % (cell,))
        idx, d2 = host(idx), host(d2)
        assert not np.isin(idx, bad).any() and (idx[bad] == -1).all() and np.isinf(d2[bad]).all()
    none = pc.PointGrid(dev(np.full((5, 3), np.nan, F)))
    assert none.n_finite == 0 and none.n_cells == 0 and (host(pc.knn(none, 3)[0]) == -1).all()
    empty = pc.PointGrid(dev(np.zeros((0, 3), F)))
    assert pc.knn(empty, 3)[0].shape == (0, 3) and pc.knn(empty, 3, queries=dev(cloud(4)))[0].tolist() == [[-1] * 3] * 4


def test_mean_distance_and_the_outlier_mask(pc):
    pts, is_out = pr.noisy_plane(1350, 150, 0)
    pts[11] = np.nan
    want_keep, want_md, want_thr = pr.outlier_mask(pts, 16, 2.0)
    grid = pc.PointGrid(dev(pts))
    md = host(pc.neighbor_mean_distance(grid, 16))
    assert md.dtype == F and np.array_equal(md.view(np.int32), want_md.view(np.int32)) and np.isnan(md[11])
    keep, md2, info = pc.statistical_outlier_mask(grid, k=16, std_ratio=2.0)
    assert keep.dtype == torch.bool and np.array_equal(host(md2).view(np.int32), md.view(np.int32))
    thr = float(info["threshold"])
    assert info["threshold"].dtype == torch.float64 and abs(thr - want_thr) <= 1e-12 * want_thr
    # the threshold comes from torch's reduction, whose order is not the restatement's: points within an f32 ulp of it
    # may fall on either side; the seed was chosen so that the restatement has at most 2 such points (it has none)
    near = np.abs(want_md.astype(np.float64) - want_thr) <= np.spacing(F(want_thr))
    print("threshold %.9g (the restatement: %.9g), %d points within an ulp of it" % (thr, want_thr, int(near.sum())))
    assert near.sum() <= 2
    assert np.array_equal(host(keep)[~near], want_keep[~near]) and not host(keep)[11]
    single = pc.PointGrid(dev(cloud(1)))
    assert np.isnan(host(pc.neighbor_mean_distance(single, 4))).all() and not host(pc.statistical_outlier_mask(single)[0]).any()


def check_normals(pc, pts, k, toward, what):
    grid = pc.PointGrid(dev(pts))
    tw = None if toward is None else dev(np.asarray(toward, F))
    nrm, var, ok, cov = (host(x) for x in pc.estimate_normals(grid, k=k, toward=tw, return_cov=True))
    idx = pr.knn(pts, k)[0]
    want = pr.normals(pts, idx, toward=toward)
    assert nrm.dtype == F and var.dtype == F and ok.dtype == np.uint8 and cov.dtype == np.float64 and cov.shape == (len(pts), 9)
    hole = np.isnan(want["cov"])                                        # (a NaN's payload is not compared)
    assert np.array_equal(np.isnan(cov), hole) and np.array_equal(cov[~hole].view(np.int64), want["cov"][~hole].view(np.int64)), what
    assert np.array_equal(ok, want["ok"]), what
    assert np.isnan(nrm[ok == 0]).all() and np.isnan(var[ok == 0]).all() and np.isfinite(nrm[ok == 1]).all(), what
    sure = (ok == 1) & (want["gap"] >= MIN_GAP)
    if sure.any():
        ang = pr.angle(nrm[sure], want["normal"][sure])
        print("%s: %d of %d normals compared, the largest angle %.3g rad" % (what, int(sure.sum()), len(pts), ang.max()))
        assert ang.max() < MAX_NORMAL_RAD, what
        assert np.abs(np.linalg.norm(nrm[sure].astype(np.float64), axis=1) - 1).max() < 2e-7, what
        assert np.abs(var[sure] - want["variation"][sure]).max() < 1e-6, what
        if toward is not None:
            assert ((nrm[sure] * want["normal"][sure]).sum(1) > 0).all(), what
            assert ((nrm[sure] * (np.asarray(toward, F).reshape(-1, 3) - pts[sure])).sum(1) > 0).all(), what
    three = pc.estimate_normals(grid, k=k, toward=tw)
    assert len(three) == 3 and np.array_equal(host(three[0]).view(np.int32), nrm.view(np.int32))
    return int(sure.sum())


def test_covariance_and_normals(pc):
    plane, is_out = pr.noisy_plane(1350, 150, 0)
    plane[5] = np.nan
    sphere, outward, centre = pr.sphere(1500, 0)
    assert check_normals(pc, plane, 16, pr.CAMERA, "plane toward the camera") > 1300
    assert check_normals(pc, sphere, 16, centre, "sphere toward its centre") > 1400
    assert check_normals(pc, sphere, 8, None, "sphere, no viewpoint") > 1400
    per_point = sphere.astype(np.float64) + 0.1 * outward                # one viewpoint per point, just outside
    assert check_normals(pc, sphere, 33, per_point.astype(F), "sphere, a viewpoint per point") > 1400
    # degenerate sets: collinear points, a single point, k = 1 (two members)
    line = np.stack([np.arange(8), np.zeros(8), np.zeros(8)], 1).astype(F)
    for pts, k in ((line, 4), (line[:1], 4), (sphere[:50], 1)):
        assert check_normals(pc, pts, k, None, "degenerate") == 0
        nrm, var, ok = pc.estimate_normals(pc.PointGrid(dev(pts)), k=k)
        assert not host(ok).any() and np.isnan(host(nrm)).all() and np.isnan(host(var)).all()


@pytest.mark.parametrize("n", [1, 257, 1500])
def test_voxel_downsample(pc, n):
    pts = cloud(n, 7)
    if n > 100:
        pts[3], pts[50, 1] = np.nan, np.inf
    attr = np.random.RandomState(n).normal(size=(n, 2)).astype(F)
    for cell in (0.13, HUGE, 1e-3):                                     # some points each, everything in one, one point each
        want = pr.voxel_downsample(pts, cell, attr)
        got = pc.voxel_downsample(dev(pts), cell, dev(attr))
        m = len(want["keys"])
        assert m == {HUGE: 1, 1e-3: np.isfinite(pts).all(1).sum()}.get(cell, m)
        for name, dtype in (("points", F), ("count", np.int32), ("cell_of_point", np.int32), ("first", np.int32),
                            ("attributes", F)):
            g = host(getattr(got, name))
            assert g.dtype == dtype and g.shape == want[name].shape, (name, cell)
            assert np.array_equal(g.view(np.int32), want[name].view(np.int32)), (name, cell)
        assert np.array_equal(host(got.grid.keys), want["keys"])
        again = pc.voxel_downsample(got.grid)                           # a PointGrid serves too, and attributes are optional
        assert again.attributes is None and torch.equal(again.points, got.points)


# ---------------------------------------------------------------------------------------------------------------------
def look_at(centre, target):
    z = (target - centre) / np.linalg.norm(target - centre)
    x = np.cross([0.0, 0.0, 1.0], z)
    x /= np.linalg.norm(x)
    R = np.stack([x, np.cross(z, x), z])
    return R, -R @ centre                                               # x_cam = R x_world + t


def corner_track(V=3, H=96, W=96, seed=0):
    """the corner scene of tests/meshreg_ref.py (three unit squares) seen V times by a camera that stands still in the
    positive octant: z-depth maps by ray / plane intersection in f64, NaN where a ray misses.  With one pose for all
    views a pixel lands on itself in every other view, so the fused depth is the rendered one and the fused points lie
    on the squares to f32 rounding (between views that differ, the nearest-pixel match of the fusion alone moves them by
    about 2e-3, beyond the noise-free thresholds).  2 % of the pixels are gross outliers in every view alike (the depth
    scaled by 0.5 .. 0.8): the fusion finds them consistent and keeps them."""
    rs = np.random.RandomState(seed)
    K, ray = fr.camera(H, W)
    R, t, depth = np.empty((1, V, 3, 3)), np.empty((1, V, 3)), np.full((1, V, H * W), np.nan)
    for v in range(V):
        R[0, v], t[0, v] = look_at(np.array([2.2, 1.9, 1.7]), np.array([0.3, 0.3, 0.3]))
    R, t = R.astype(F), t.astype(F)
    for v in range(V):
        Rm, tv = R[0, v].astype(np.float64), t[0, v].astype(np.float64)
        o, dirs = -Rm.T @ tv, ray.astype(np.float64) @ Rm               # X_world = o + d (R^T ray)
        best = np.full(H * W, np.inf)
        for axis in range(3):
            with np.errstate(all="ignore"):
                d = -o[axis] / dirs[:, axis]
            X = o + d[:, None] * dirs
            a, b = X[:, (axis + 1) % 3], X[:, (axis + 2) % 3]
            hit = (d > 0) & (a >= 0) & (a <= 1) & (b >= 0) & (b <= 1) & (d < best)
            best = np.where(hit, d, best)
        depth[0, v] = np.where(np.isfinite(best), best, np.nan)
    gross = rs.rand(H * W) < 0.02
    depth = np.where(gross, depth * rs.uniform(0.5, 0.8, H * W), depth)
    return depth.reshape(1, V, H, W).astype(F), ray, K, R, t


def test_fused_points_to_a_registered_pose(pc):
    """depth_fuse_points -> outlier mask -> normals toward the view centres -> robust_mesh_icp(normals=, min_cos=0.5) on
    the corner mesh moved by 5 degrees and 0.03: the outputs have the shapes and conventions the consumer expects, and
    the pose ends within the noise-free thresholds of tests/test_mesh_register_host.py"""
    from connecting_the_dots_amd import meshrobust
    from connecting_the_dots_amd.torchext import functions as fn
    depth, ray, K, R, t = corner_track()
    V, H, W = depth.shape[1:]
    points, src, n_per_track = fn.depth_fuse_points(dev(depth), dev(ray), dev(K), dev(R), dev(t))
    assert int(n_per_track[0]) == len(points) > 2000
    grid = pc.PointGrid(points)
    keep, mean_dist, info = pc.statistical_outlier_mask(grid, k=16, std_ratio=2.0)
    centers = pc.view_centers(src, dev(R), dev(t), (V, H, W))
    assert centers.shape == points.shape and centers.dtype == torch.float32
    kept = points[keep].contiguous()
    normals, variation, ok = pc.estimate_normals(pc.PointGrid(kept), k=16, toward=centers[keep].contiguous())
    good = ok.bool()
    kept, normals = kept[good].contiguous(), normals[good].contiguous()
    on_surface = (kept.abs().amin(dim=1) < 1e-4)                        # the squares are the planes x, y, z = 0
    # the squares' face normals point along +axis, to the cameras: away from a rim every normal is within a few degrees
    inside = on_surface & (kept.abs().sort(dim=1).values[:, 1] > 0.15)
    assert int(inside.sum()) > 1000 and float((normals[inside].amax(dim=1) > 0.99).float().mean()) > 0.95
    verts, faces = mr.corner_mesh()
    Q = mr.rotation([0.3, -0.5, 0.8], 5.0)
    d = np.array([0.02, -0.01, 0.02])
    moved = (verts.astype(np.float64) @ Q.T + d).astype(F)             # the pose that lays the points on it is (Q, d)
    Rr, tr, icp = meshrobust.robust_mesh_icp(kept, dev(moved), dev(faces), iters=20, scale=0.05, normals=normals, min_cos=0.5,
                                             max_dist=0.25)
    rot, shift = mr.pose_error(host(Rr), host(tr), Q, d)
    print("%d fused points, %d kept, %d with a normal; the pose ends %.3e degrees, %.3e off; used %s" % (
        len(points), int(keep.sum()), len(kept), rot, shift, host(icp["used"])[-1]))
    assert int(icp["ok"]) == 1
    assert rot < MAX_ROT_DEG and shift < MAX_T
