"""CPU checks of the point-cloud family (include/ext/ctd_hip_point_cloud.h, pointcloud) as tests/pointcloud_ref.py states
it: the header's prototypes against pointcloud's table and the library, that the pinned interface lists did not move,
every rejection of the C entry points (through the library, no GPU needed: each returns before any HIP call) and of the
Python checks, the kNN rule by hand, and that the outlier filter and the normals do their job in the restatement.

Measured from the restatement on the CPU (seed 0; the bounds below lie half-way between the figure and chance):
  noisy plane, 1350 inliers + 150 uniform gross outliers (9 : 1), k = 16, std_ratio = 2: 82.67 % of the outliers removed
    (seeds 1 to 3: 78.7, 78.0, 79.3) -> bound (82.67 + 50) / 2 = 66.3 %; 100.00 % of the inliers kept -> bound 75 %.
  normals, k = 16, median angle to the analytic normal: noisy plane (the 1350 inliers) 2.76 degrees, sphere of 1500
    points 1.28 degrees; a random direction: 60 degrees (measured 59.94 over 10^5 draws) -> bounds 31.4 and 30.6 degrees."""
import ctypes
import glob
import os
import re

import numpy as np
import pytest

from tests import pointcloud_ref as pr
from tests.abi_headers import parse_header

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ext", "ctd_hip_point_cloud.h")
NAMES = ["ctd_point_cell_keys_f32", "ctd_point_knn_f32", "ctd_point_mean_dist_f32", "ctd_point_normals_f32",
         "ctd_point_voxel_mean_f32"]

C_SCALARS = {"int": ctypes.c_int, "float": ctypes.c_float, "size_t": ctypes.c_size_t, "int64_t": ctypes.c_int64}

N_IN, N_OUT, SEED = 1350, 150, 0
MIN_OUTLIERS_REMOVED = (0.8267 + 0.5) / 2
MIN_INLIERS_KEPT = (1.0 + 0.5) / 2
RANDOM_DEG = 60.0                                      # the median angle between a fixed and a random direction, up to sign
MAX_PLANE_DEG = (2.76 + RANDOM_DEG) / 2
MAX_SPHERE_DEG = (1.28 + RANDOM_DEG) / 2


def test_header_matches_the_module_table_and_the_library():
    from connecting_the_dots_amd import _lib, pointcloud
    functions, structs = parse_header(HEADER)
    assert not structs and list(functions) == list(pointcloud.TABLE) == NAMES
    bound = pointcloud.lib()
    assert bound is _lib.lib()
    for name, (ret, params) in functions.items():
        res, args = pointcloud.TABLE[name]
        assert res is C_SCALARS[ret], name
        assert len(args) == len(params), name
        for i, (ctype, declared) in enumerate(zip(args, params)):
            assert (ctype is ctypes.c_void_p) if declared.endswith("*") else (ctype is C_SCALARS[declared]), (name, i)
        assert getattr(bound, name).argtypes == args and getattr(bound, name).restype == res, name
    text = open(HEADER).read()
    assert re.findall(r'#\s*include\s*[<"]([^>"]+)[>"]', text) == ["../ctd_hip.h"]
    assert "((dx * dx) + (dy * dy)) + (dz * dz)" in text and "the lower index winning a tie" in text
    assert "((dx * dx) + (dy * dy)) + (dz * dz)" in pointcloud.knn.__doc__


def test_the_pinned_interface_did_not_move():
    from connecting_the_dots_amd import _lib, build, meshglobal, meshreg, meshrobust, pointcloud, torchext
    headers = sorted(os.path.basename(p) for p in glob.glob(os.path.join(ROOT, "include", "*.h")))
    assert headers == sorted(_lib.TABLES) and len(headers) == 14
    assert pointcloud.HEADER not in _lib.TABLES and pointcloud.TABLE not in _lib.TABLES.values()
    assert not any(name in table for table in _lib.TABLES.values() for name in pointcloud.TABLE)
    assert not any(name in other.TABLE for other in (meshglobal, meshreg, meshrobust) for name in pointcloud.TABLE)
    assert len(torchext.functions.__all__) == 65
    assert not any(n in torchext.functions.__all__ for n in (
        "PointGrid", "knn", "neighbor_mean_distance", "statistical_outlier_mask", "estimate_normals", "view_centers",
        "voxel_downsample"))
    assert HEADER in build._headers()                                   # a stale header rebuilds
    assert _lib.lib().ctd_version() == 5


INVALID, UNSUPPORTED = 1, 3


def _regions():
    buf = ctypes.create_string_buffer(1 << 17)
    base = (ctypes.addressof(buf) + 255) // 256 * 256
    return buf, [base + 4096 * i for i in range(24)]         # disjoint 4 KiB host regions: never dereferenced


def _walk(call, classes):
    """each class of error wins over every later one: pair it with a later error and the answer does not change"""
    for i, group in enumerate(classes):
        for bad, want in group:
            assert call(**bad) == want, bad
            for later in classes[i + 1:]:
                assert call(**{**later[0][0], **bad}) == want, (bad, later[0][0])


def test_the_entry_points_validate_before_any_hip_call():
    from connecting_the_dots_amd import pointcloud
    L = pointcloud.lib()
    keep, p = _regions()
    nan, inf = float("nan"), float("inf")
    I, U = INVALID, UNSUPPORTED

    def keys(points=p[0], n=10, ox=0.0, oy=0.0, oz=0.0, cell=0.5, out=p[1]):
        return L.ctd_point_cell_keys_f32(points, n, ox, oy, oz, cell, out, -1, None)

    _walk(keys, [
        [(dict(n=-1), I), (dict(n=-(1 << 31)), I)],
        [(dict(cell=v), I) for v in (0.0, -1.0, nan, inf, -inf)] + [(dict(ox=nan), I), (dict(oy=inf), I), (dict(oz=-inf), I)],
        [(dict(points=None), I), (dict(out=None), I)],
        [(dict(out=p[0]), I), (dict(out=p[0] + 112), I), (dict(out=p[0] - 72), I)],
    ])
    assert keys(n=0, points=None, out=None) == 0                        # nothing to do: CTD_OK without a launch
    assert keys(n=0, cell=nan) == I

    def knn(pts=p[0], order=p[1], ns=10, keys=p[2], start=p[3], nc=4, dx=3, dy=4, dz=5, ox=0.0, oy=0.0, oz=0.0, cell=0.5,
            queries=p[4], nq=7, k=16, md2=inf, idx=p[5], d2=p[6]):
        return L.ctd_point_knn_f32(pts, order, ns, keys, start, nc, dx, dy, dz, ox, oy, oz, cell, queries, nq, k, md2, idx, d2,
                                   -1, None)

    _walk(knn, [
        [(dict(ns=-1), I), (dict(nc=-1), I), (dict(nq=-1), I), (dict(nc=11), I), (dict(nc=0), I), (dict(ns=0), I)],
        [(dict(k=0), I), (dict(k=65), I), (dict(k=-1), I)],
        [(dict(dx=0), I), (dict(dy=0), I), (dict(dz=-1), I), (dict(dx=(1 << 21) + 1), I), (dict(dz=(1 << 21) + 1), I)],
        [(dict(cell=v), I) for v in (0.0, -1.0, nan, inf)] + [(dict(ox=nan), I), (dict(oz=inf), I)],
        [(dict(md2=nan), I), (dict(md2=-1.0), I), (dict(md2=-inf), I)],
        [(dict(nq=1 << 27, k=16), U), (dict(nq=(1 << 31) - 1, k=64), U)],
        [(dict(queries=None, nq=9), I)],
        [(dict(idx=None), I), (dict(d2=None), I), (dict(pts=None), I), (dict(order=None), I), (dict(keys=None), I),
         (dict(start=None), I), (dict(queries=None, nq=10, order=None), I)],
        [(dict(idx=p[6]), I), (dict(d2=p[0]), I), (dict(idx=p[1] + 36), I), (dict(d2=p[2] + 24), I), (dict(idx=p[3] + 16), I),
         (dict(d2=p[4] + 80), I), (dict(idx=p[4] - 444), I)],
    ])
    assert knn(nq=0, idx=None, d2=None) == 0 and knn(nq=0, k=0) == I
    assert knn(dx=1 << 21, dy=1 << 21, dz=1 << 21, k=64, md2=0.0, idx=None) == I      # the limits pass: the NULL answers
    assert knn(ns=0, nc=0, pts=None, order=None, keys=None, start=None, idx=None) == I  # an empty grid needs no tables

    def mean(d2=p[0], n=10, k=16, out=p[1]):
        return L.ctd_point_mean_dist_f32(d2, n, k, out, -1, None)

    _walk(mean, [
        [(dict(n=-1), I), (dict(k=0), I), (dict(k=65), I)],
        [(dict(n=1 << 27), U)],
        [(dict(d2=None), I), (dict(out=None), I)],
        [(dict(out=p[0]), I), (dict(out=p[0] + 636), I), (dict(out=p[0] - 36), I)],
    ])
    assert mean(n=0, d2=None, out=None) == 0

    def normals(pts=p[0], n=10, idx=p[1], k=16, toward=p[2], stride=3, nrm=p[3], var=p[4], ok=p[5], cov=p[6]):
        return L.ctd_point_normals_f32(pts, n, idx, k, toward, stride, nrm, var, ok, cov, -1, None)

    _walk(normals, [
        [(dict(n=-1), I), (dict(k=0), I), (dict(k=65), I), (dict(stride=1), I), (dict(stride=-3), I), (dict(stride=6), I)],
        [(dict(n=1 << 27), U)],
        [(dict(pts=None), I), (dict(idx=None), I), (dict(nrm=None), I), (dict(var=None), I), (dict(ok=None), I)],
        [(dict(nrm=p[0]), I), (dict(var=p[1] + 636), I), (dict(ok=p[2] + 119), I), (dict(cov=p[3] + 112), I),
         (dict(var=p[3]), I), (dict(cov=p[5] - 712), I), (dict(stride=0, ok=p[2] + 11), I)],
    ])
    assert normals(n=0, pts=None, idx=None, nrm=None, var=None, ok=None, cov=None) == 0
    assert normals(toward=None, stride=0, cov=None, nrm=None) == I      # toward and cov are optional: the NULL normals answer
    assert normals(stride=0, ok=p[2] + 12, nrm=None) == I               # one viewpoint is 12 bytes: no overlap, the NULL answers

    def voxel(values=p[0], n=10, C=3, order=p[1], start=p[2], m=4, out=p[3]):
        return L.ctd_point_voxel_mean_f32(values, n, C, order, start, m, out, -1, None)

    _walk(voxel, [
        [(dict(n=-1), I), (dict(m=-1), I), (dict(C=0), I), (dict(C=65), I)],
        [(dict(n=1 << 30), U), (dict(m=1 << 30), U)],
        [(dict(values=None), I), (dict(order=None), I), (dict(start=None), I), (dict(out=None), I)],
        [(dict(out=p[0]), I), (dict(out=p[0] + 116), I), (dict(out=p[2] + 16), I), (dict(out=p[2] - 44), I)],
    ])
    assert voxel(m=0, values=None, order=None, start=None, out=None) == 0
    del keep


def test_the_module_checks_its_arguments_without_a_gpu():
    import torch
    from connecting_the_dots_amd import pointcloud as pc
    cpu = torch.zeros((4, 3))
    for bad in (None, cpu, cpu.double(), [[0.0, 0.0, 0.0]]):
        with pytest.raises(RuntimeError):
            pc.PointGrid(bad)                                           # no CPU path: a tensor that is not CUDA is refused
        with pytest.raises(RuntimeError):
            pc.voxel_downsample(bad, 0.1)
    for call in (lambda g: pc.knn(g, 4), lambda g: pc.neighbor_mean_distance(g, 4), pc.statistical_outlier_mask,
                 pc.estimate_normals, lambda g: pc.voxel_downsample(g, 0.1, cpu)):
        for bad in (None, cpu, "grid"):
            with pytest.raises(RuntimeError):
                call(bad)
    grid = object.__new__(pc.PointGrid)                                 # the checks that come before any tensor is touched
    for k in (0, 65, -1, 2.0, True, None):
        with pytest.raises(RuntimeError):
            pc.knn(grid, k)
    for md in (-1.0, float("nan"), float("inf"), "1", True):
        with pytest.raises(RuntimeError):
            pc.knn(grid, 4, max_dist=md)
    with pytest.raises(RuntimeError):
        pc.statistical_outlier_mask(grid, std_ratio=float("nan"))
    with pytest.raises(RuntimeError):
        pc.estimate_normals(grid, return_cov=1)
    src, R, t = torch.zeros(5, dtype=torch.int64), torch.zeros((1, 2, 3, 3)), torch.zeros((1, 2, 3))
    for bad in (dict(src=src.int()), dict(src=src[None]), dict(shape=(2, 4)), dict(shape=(3, 4, 4)), dict(shape=(2, 0, 4)),
                dict(t=t[0])):
        with pytest.raises(RuntimeError):
            pc.view_centers(**{**dict(src=src, R=R, t=t, shape=(2, 4, 4)), **bad})
    # view_centers is torch ops only: -t @ R of the view of each index, checked here on the CPU
    rs = np.random.RandomState(0)
    R = torch.from_numpy(np.linalg.qr(rs.normal(size=(2, 3, 3, 3)))[0].astype(F))
    t = torch.from_numpy(rs.normal(size=(2, 3, 3)).astype(F))
    V, H, W = 3, 4, 5
    src = torch.from_numpy(rs.randint(0, 2 * V * H * W, 50))
    got = pc.view_centers(src, R, t, (V, H, W)).numpy()
    b, r = src.numpy() // (V * H * W), (src.numpy() // (H * W)) % V
    want = -np.einsum("ni,nij->nj", t.numpy()[b, r].astype(np.float64), R.numpy()[b, r].astype(np.float64))
    assert got.dtype == F and np.abs(got - want).max() < 1e-6
    assert pc.PointGrid._check_extent(1.0, 1e-3, "t") is None
    with pytest.raises(RuntimeError, match="2\\^21"):
        pc.PointGrid._check_extent(1.0, 1e-7, "t")


# ---------------------------------------------------------------------------------------------------------------------
def test_the_knn_rule_by_hand():
    nan = np.nan
    pts = np.array([[0, 0, 0], [1, 0, 0], [-1, 0, 0], [0, 2, 0], [nan, 0, 0], [0, 0, 0], [0, 0, 3]], F)
    idx, d2 = pr.knn(pts, 3)
    assert idx.dtype == np.int32 and d2.dtype == F
    assert idx[0].tolist() == [5, 1, 2] and d2[0].tolist() == [0, 1, 1]          # the coincident point first, then a tie by index
    assert idx[5].tolist() == [0, 1, 2] and d2[5].tolist() == [0, 1, 1]          # each of the pair lists the other, not itself
    assert idx[1].tolist() == [0, 5, 2] and d2[1].tolist() == [1, 1, 4]
    assert idx[3].tolist() == [0, 5, 1] and d2[3].tolist() == [4, 4, 5]
    assert idx[4].tolist() == [-1] * 3 and np.isinf(d2[4]).all()                 # a NaN point has no neighbours ...
    assert not (idx == 4).any()                                                  # ... and is nobody's
    assert all(i not in idx[i] for i in range(len(pts)))
    # padding: 5 other finite points, k = 8
    idx, d2 = pr.knn(pts, 8)
    assert idx[6].tolist() == [0, 5, 1, 2, 3, -1, -1, -1] and d2[6, :5].tolist() == [9, 9, 10, 10, 13] and np.isinf(d2[6, 5:]).all()
    # max_dist counts d2 <= max_dist^2 inclusively, squared in f32
    idx, d2 = pr.knn(pts, 3, max_dist=1.0)
    assert idx[0].tolist() == [5, 1, 2] and idx[3].tolist() == [-1, -1, -1] and idx[1].tolist() == [0, 5, -1]
    idx, d2 = pr.knn(pts, 2, max_dist=0.0)
    assert idx[0].tolist() == [5, -1] and idx[1].tolist() == [-1, -1]
    # separate queries exclude nothing; one that is not finite is empty
    idx, d2 = pr.knn(pts, 2, queries=np.array([[0, 0, 0], [0.5, 0, 0], [np.inf, 0, 0]], F))
    assert idx.tolist() == [[0, 5], [0, 1], [-1, -1]] and d2[:2].tolist() == [[0, 0], [0.25, 0.25]]
    # the association: ((dx dx) + (dy dy)) + (dz dz) in f32, not the f64 sum rounded
    q, p = np.array([[0.1, 0.2, 0.3]], F), np.array([[1.7, -2.9, 4.1]], F)
    dx, dy, dz = (p - q)[0]
    assert pr.knn(p, 1, queries=q)[1][0, 0] == F(F(F(dx * dx) + F(dy * dy)) + F(dz * dz))
    assert pr.knn(np.zeros((0, 3), F), 2)[0].shape == (0, 2)
    # the consumers on the same points
    md = pr.mean_dist(pr.knn(pts, 3)[1])
    assert md[0] == F(2 / 3) and np.isnan(md[4]) and md[3] == F((2.0 + 2.0 + np.sqrt(5.0)) / 3)
    v = pr.voxel_downsample(pts, 1.5, pts[:, :1] * 2)
    assert v["cell_of_point"].tolist() == [0, 1, 0, 2, -1, 0, 3] and v["count"].tolist() == [3, 1, 1, 1]
    assert v["first"].tolist() == [0, 1, 3, 6] and v["points"][0].tolist() == [F(-1 / 3), 0, 0]
    assert v["attributes"][:, 0].tolist() == [F(-2 / 3), 2, 0, 0] and (np.diff(v["keys"]) > 0).all()


def test_the_outlier_filter_does_its_job_in_the_restatement():
    pts, is_out = pr.noisy_plane(N_IN, N_OUT, SEED)
    assert (~is_out).sum() >= 5 * is_out.sum()                          # otherwise mean + 2 std is no meaningful threshold
    keep, md, threshold = pr.outlier_mask(pts, k=16, std_ratio=2.0)
    removed, kept = float((~keep[is_out]).mean()), float(keep[~is_out].mean())
    print("outliers removed %.4f, inliers kept %.4f, threshold %.5f" % (removed, kept, threshold))
    assert removed >= MIN_OUTLIERS_REMOVED and kept >= MIN_INLIERS_KEPT
    # a NaN point has a NaN mean and is not kept
    pts[7] = np.nan
    keep, md, _ = pr.outlier_mask(pts, k=16)
    assert np.isnan(md[7]) and not keep[7] and np.isfinite(np.delete(md, 7)).all()


def test_the_normals_do_their_job_in_the_restatement():
    pts, is_out = pr.noisy_plane(N_IN, N_OUT, SEED)
    inl = pts[~is_out]
    r = pr.normals(inl, pr.knn(inl, 16)[0], toward=pr.CAMERA)
    plane = float(np.degrees(np.median(pr.angle(r["normal"], pr.PLANE_N))))
    sp, outward, centre = pr.sphere(1500, SEED)
    s = pr.normals(sp, pr.knn(sp, 16)[0], toward=centre)
    ball = float(np.degrees(np.median(pr.angle(s["normal"], outward))))
    print("median angle to the analytic normal: plane %.3f degrees, sphere %.3f" % (plane, ball))
    assert r["ok"].all() and s["ok"].all()
    assert plane <= MAX_PLANE_DEG and ball <= MAX_SPHERE_DEG
    assert (((pr.CAMERA - inl) * r["normal"]).sum(1) > 0).all()         # every normal points to the camera ...
    assert ((s["normal"] * outward).sum(1) < 0).all()                   # ... or to the centre: inward
    assert np.abs(np.linalg.norm(r["normal"], axis=1) - 1).max() < 1e-12
    assert ((s["variation"] >= 0) & (s["variation"] <= 1 / 3)).all()
    # degenerate sets: a line, a single point, k = 1 (two members)
    line = np.stack([np.arange(8), np.zeros(8), np.zeros(8)], 1).astype(F)
    for p, k in ((line, 4), (line[:1], 4), (sp[:50], 1)):
        d = pr.normals(p, pr.knn(p, k)[0])
        assert not d["ok"].any() and np.isnan(d["normal"]).all() and np.isnan(d["variation"]).all()
