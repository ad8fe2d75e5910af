"""GPU parity of the global point-to-mesh registration (meshglobal.pose_scores, distance_levels, best_starts,
global_mesh_icp, global_aligned_reconstruction_error; include/ext/ctd_hip_mesh_global.h) against tests/meshglobal_ref.py.

The score is an exact integer, so pose_scores equals the restatement with torch.equal at every shape, whatever the order
of the points; distance_levels equals the reference's levels at every voxel (both rest on the nearest-face distance whose
bits the project pins).  global_mesh_icp meets the thresholds of tests/test_mesh_global_host.py on its scene, where
meshreg.mesh_icp from the identity ends more than 30 degrees off, and two runs give the same bits."""
import numpy as np
import pytest
import torch

from tests import meshglobal_ref as gr
from tests import meshreg_ref as mr
from tests.test_mesh_global_host import FAR_DEG, MAX_ROT_DEG, MAX_T
from tests.test_mesh_register_gpu import bits, dev, host

pytestmark = pytest.mark.gpu

F = np.float32
DIMS = (7, 9, 11)                                     # nx, ny, nz: all different, so that a swapped axis shows
ORIGIN, VOXEL = (-0.75, -1.0, -1.25), 0.25            # exact in f32, and so is every half-voxel boundary
M_ROT = 37


@pytest.fixture(scope="module")
def mgl():
    from connecting_the_dots_amd import meshglobal
    return meshglobal


def small_volume(seed=0):
    """levels uint8 [11,9,7] with every value from 0 to 255 in it, 0 and 255 many times"""
    rs = np.random.RandomState(seed)
    levels = rs.randint(0, 256, size=DIMS[::-1]).astype(np.uint8)
    levels[rs.rand(*levels.shape) < 0.1] = 0
    levels[rs.rand(*levels.shape) < 0.1] = 255
    return levels


def small_poses():
    """pose 0 is the identity with base 0 (under it the half-voxel points stay exact); the others turn about the centre of
    the volume"""
    R = gr.rotation_grid(M_ROT)
    R[0] = np.eye(3, dtype=F)
    c = np.array(ORIGIN, np.float64) + VOXEL * (np.array(DIMS) - 1) / 2.0
    base = (c[None] - R.astype(np.float64) @ c).astype(F)
    base[0] = 0
    return R, np.ascontiguousarray(base)


def small_points(n, seed):
    """n points around the volume: uniform in a box that the volume fills to two thirds (a third land outside under the
    identity); every 5th has a coordinate exactly on a half-voxel boundary (u + 0.5 an integer), the boundaries g = 0
    and g = dim among them; every 17th is NaN or +-inf in one coordinate"""
    rs = np.random.RandomState(seed)
    lo = np.array(ORIGIN) - VOXEL / 2
    size = VOXEL * np.array(DIMS)
    grow = (1.5 ** (1.0 / 3.0) - 1.0) / 2.0
    P = (lo - grow * size + rs.rand(n, 3) * size * (1 + 2 * grow)).astype(F)
    k = np.arange(n)
    on = k % 5 == 1
    axis = rs.randint(0, 3, size=n)
    cell = np.stack([rs.randint(-1, d + 1, size=n) for d in DIMS], 1)                   # -1 .. dim: the outer boundaries too
    edge = (np.array(ORIGIN) + VOXEL * (cell - 0.5)).astype(F)                          # exact: multiples of 0.125
    P[on, axis[on]] = edge[on, axis[on]]
    bad = k % 17 == 3
    P[bad, axis[bad]] = np.array([np.nan, np.inf, -np.inf], F)[k[bad] % 3]
    return np.ascontiguousarray(P)


_SMALL = {}


def small_case(n, T):
    """(points, R, base, offsets, levels, the restatement's scores), computed once and shared (read-only)"""
    if (n, T) not in _SMALL:
        R, base = small_poses()
        steps = {1: 1, 8: 2, 27: 3}.get(T)
        offsets = gr.offset_grid(steps, 0.3) if steps else np.ascontiguousarray(gr.offset_grid(3, 0.3)[3:3 + T])
        pts, levels = small_points(n, n + T), small_volume()
        want = gr.pose_scores(pts, R, base, offsets, levels, ORIGIN, VOXEL)
        _SMALL[(n, T)] = (pts, R, base, offsets, levels, want)
    return _SMALL[(n, T)]


def test_the_small_points_are_what_they_claim():
    pts, R, base, offsets, levels, _ = small_case(1500, 1)
    u = (pts.astype(np.float64) - np.array(ORIGIN)) / VOXEL + 0.5
    with np.errstate(invalid="ignore"):
        inside = ((np.floor(u) >= 0) & (np.floor(u) < np.array(DIMS))).all(1)
        on_boundary = (u == np.floor(u)).any(1)
    assert 0.25 < 1 - inside.mean() < 0.45 and on_boundary.sum() >= 250
    assert (on_boundary & inside).sum() > 50 and (on_boundary & ~inside).sum() > 50
    assert np.isnan(pts).any() and np.isposinf(pts).any() and np.isneginf(pts).any()
    assert (levels == 0).sum() > 30 and (levels == 255).sum() > 30 and len(np.unique(levels)) > 200


@pytest.mark.parametrize("T", [1, 5, 8, 9, 27])
@pytest.mark.parametrize("n", [1, 255, 257, 1500])
def test_pose_scores_equal_the_restatement(mgl, n, T):
    pts, R, base, offsets, levels, want = small_case(n, T)
    args = [dev(pts), dev(R), dev(base), dev(offsets), dev(levels), dev(np.array(ORIGIN, F))]
    before = [x.clone() for x in args]
    got = mgl.pose_scores(*args, VOXEL)
    assert got.dtype == torch.int64 and got.shape == (M_ROT, T)
    differ = host(got) != want
    assert not differ.any(), "%d of %d scores differ, first at %s: %d vs %d" % (
        int(differ.sum()), differ.size, np.argwhere(differ)[0], host(got)[differ][0], want[differ][0])
    assert all(torch.equal(bits(x), bits(y)) for x, y in zip(args, before)), "an input was written"
    assert torch.equal(mgl.pose_scores(*args, VOXEL, order=None), got)


def test_the_order_of_the_points_changes_no_bit(mgl):
    pts, R, base, offsets, levels, want = small_case(1500, 27)
    rest = [dev(R), dev(base), dev(offsets), dev(levels), dev(np.array(ORIGIN, F))]
    shuffled = pts[np.random.RandomState(5).permutation(len(pts))]
    for p in (pts, shuffled, pts[::-1].copy()):
        for order in (None, "morton"):
            assert np.array_equal(host(mgl.pose_scores(dev(p), *rest, VOXEL, order=order)), want), order
    perm = host(mgl.morton_order(dev(pts)))
    assert sorted(perm.tolist()) == list(range(len(pts)))
    assert not np.isfinite(pts[perm[-(~np.isfinite(pts).all(1)).sum():]]).all(1).any()   # the points that are not finite go last
    with pytest.raises(RuntimeError):
        mgl.pose_scores(dev(pts), *rest, VOXEL, order="hilbert")


def test_the_overflow_bound_and_the_edges(mgl):
    R, base = small_poses()
    origin = dev(np.array(ORIGIN, F))
    levels = dev(small_volume())
    zero = dev(np.zeros((1, 3), F))
    # 65536 points, all outside: 65536 * 255^2 = 4261478400 needs the 33rd bit of a signed sum and fits an unsigned one
    far = dev(np.full((65536, 3), 100.0, F))
    got = mgl.pose_scores(far, dev(R[:2]), dev(base[:2]), zero, levels, origin, VOXEL)
    assert got.tolist() == [[4261478400], [4261478400]]
    with pytest.raises(RuntimeError):
        mgl.pose_scores(dev(np.zeros((65537, 3), F)), dev(R[:2]), dev(base[:2]), zero, levels, origin, VOXEL)
    # no points: zeros
    none = torch.empty((0, 3), device="cuda")
    got = mgl.pose_scores(none, dev(R), dev(base), dev(gr.offset_grid(2, 0.3)), levels, origin, VOXEL)
    assert got.shape == (M_ROT, 8) and not got.any()
    # a volume of one voxel, of level 7, around (1, 2, 3): half a voxel to every side, the lower boundary inside
    one = dev(np.full((1, 1, 1), 7, np.uint8))
    pts = np.array([[1, 2, 3], [1.49, 2.49, 3.49], [0.5, 1.5, 2.5], [1.5, 2, 3], [1, 2, 3.5], [0.49, 2, 3], [np.nan, 2, 3]], F)
    got = mgl.pose_scores(dev(pts), dev(R[:1]), dev(base[:1]), zero, one, dev(np.array([1, 2, 3], F)), 1.0)
    assert got.tolist() == [[3 * 49 + 4 * 255 * 255]]
    assert np.array_equal(host(got), gr.pose_scores(pts, R[:1], base[:1], np.zeros((1, 3), F), np.full((1, 1, 1), 7, np.uint8),
                                                     (1, 2, 3), 1.0))


def test_best_starts_equal_the_restatement(mgl):
    pts, R, base, offsets, levels, want = small_case(1500, 27)
    score = want // 65025                                                # coarse: many ties, over the offsets and the rotations
    assert len(np.unique(score.min(1))) < M_ROT
    for K in (1, 8, M_ROT):
        got = mgl.best_starts(dev(score), dev(R), dev(base), dev(offsets), K)
        for g, w in zip(got, gr.best_starts(score, R, base, offsets, K)):
            assert np.array_equal(host(g), w)


# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scene_levels(mgl):
    verts, faces = gr.scaled_corner()
    origin = dev(np.array(gr.ORIGIN, F))
    return mgl.distance_levels(dev(verts), dev(faces), origin, gr.VOXEL, gr.DIMS, gr.TRUNC), origin


def test_distance_levels_equal_the_reference(mgl, scene_levels):
    levels, origin = scene_levels
    want = gr.scene_levels()
    assert levels.dtype == torch.uint8 and tuple(levels.shape) == want.shape and levels.is_contiguous()
    differ = host(levels) != want
    assert not differ.any(), "%d of %d voxels differ, the first at %s: %d vs %d" % (
        int(differ.sum()), differ.size, np.argwhere(differ)[0], host(levels)[differ][0], want[differ][0])
    verts, faces = gr.scaled_corner()
    assert torch.equal(mgl.distance_levels(dev(verts), dev(faces), origin, gr.VOXEL, gr.DIMS, gr.TRUNC, bvh=None), levels)
    # the default box: the longest padded side has `resolution` voxels and the mesh lies `pad` voxels inside
    o, voxel, dims = mgl.default_box(dev(verts), resolution=40, pad=6)
    assert dims == (40, 32, 26) and abs(voxel - 1.0 / 27) < 1e-9 and np.allclose(host(o), -6.0 / 27, atol=1e-6)


def scene_kwargs(levels, origin):
    return dict(n_rotations=gr.N_ROT, t_steps=gr.T_STEPS, t_step=gr.T_STEP, levels=levels, origin=origin, voxel=gr.VOXEL,
                K=gr.K_STARTS, iters=gr.ITERS, metric="point")


def flat_tensors(x, path=""):
    """every tensor of a nested result, with its path"""
    if isinstance(x, torch.Tensor):
        yield path, x
    elif isinstance(x, dict):
        for k in sorted(x):
            yield from flat_tensors(x[k], path + "/" + k)
    elif isinstance(x, (tuple, list)):
        for i, v in enumerate(x):
            yield from flat_tensors(v, path + "/%d" % i)


@pytest.mark.parametrize("seed", gr.SCENE_SEEDS)
def test_global_mesh_icp_finds_the_pose(mgl, scene_levels, seed):
    from connecting_the_dots_amd import meshreg
    levels, origin = scene_levels
    sc = gr.make_scene(seed)
    pts, verts, faces = dev(sc["points"]), dev(sc["verts"]), dev(sc["faces"])
    R, t, info = mgl.global_mesh_icp(pts, verts, faces, **scene_kwargs(levels, origin))
    rot, tr = mr.pose_error(host(R), host(t), sc["R_true"], sc["t_true"])
    starts = [mr.pose_error(host(info["start_R"][k]), host(info["start_t"][k]), sc["R_true"], sc["t_true"])
              for k in range(gr.K_STARTS)]
    print("seed %d: %.4f degrees / %.2e, best %d, starts %s" % (seed, rot, tr, int(info["best"]),
                                                                  ", ".join("%.1f / %.2f" % s for s in starts)))
    assert R.shape == (3, 3) and t.shape == (3,) and info["R"].shape == (gr.K_STARTS, 3, 3)
    assert int(info["ok"][info["best"]]) == 1
    assert rot < MAX_ROT_DEG and tr < MAX_T
    assert any(s[0] < gr.BASIN_DEG and s[1] < gr.BASIN_T for s in starts)              # a start in the basin among the K
    assert float(info["final"][info["best"]]) == float(info["final"].min()) and len(set(info["start_rot"].tolist())) == gr.K_STARTS
    # the local method alone, from the identity, on the same tensors
    Rp, tp, ip = meshreg.mesh_icp(pts, verts, faces, iters=gr.ITERS, metric="point")
    rot_p, tr_p = mr.pose_error(host(Rp), host(tp), sc["R_true"], sc["t_true"])
    print("seed %d: mesh_icp from the identity ends %.1f degrees / %.2f off, ok = %d" % (seed, rot_p, tr_p, int(ip["ok"])))
    assert rot_p > FAR_DEG
    # two runs: the same bits of R, t and every tensor of info
    again = mgl.global_mesh_icp(pts, verts, faces, **scene_kwargs(levels, origin))
    first, second = list(flat_tensors((R, t, info))), list(flat_tensors(again))
    assert [p for p, _ in first] == [p for p, _ in second] and len(first) >= 14
    for (path, a), (_, b) in zip(first, second):
        assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(bits(a), bits(b)), path


def test_global_mesh_icp_builds_its_own_volume(mgl):
    """the defaults (the box around the mesh, trunc = 6 voxels, offsets of 2 voxels) at 1024 rotations"""
    sc = gr.make_scene(1)
    R, t, info = mgl.global_mesh_icp(dev(sc["points"]), dev(sc["verts"]), dev(sc["faces"]), n_rotations=gr.N_ROT)
    rot, tr = mr.pose_error(host(R), host(t), sc["R_true"], sc["t_true"])
    print("defaults, seed 1: %.4f degrees / %.2e" % (rot, tr))
    assert rot < MAX_ROT_DEG and tr < MAX_T


def test_global_aligned_reconstruction_error(mgl):
    """the scaled corner of 12 x 12 quads a square, moved by 140 degrees and 0.5, against itself"""
    verts, faces = gr.scaled_corner(12)
    rs = np.random.RandomState(11)
    Q = mr.rotation(rs.normal(size=3), 140.0)
    d = rs.normal(size=3)
    d = d / np.linalg.norm(d) * 0.5
    c = verts.astype(np.float64).mean(0)
    moved = ((verts.astype(np.float64) - c) @ Q.T + c + d).astype(F)
    R_true, t_true = Q.T, c - Q.T @ (c + d)
    tv, tf = dev(verts), dev(faces)
    origin = dev(np.array(gr.ORIGIN, F))
    levels = mgl.distance_levels(tv, tf, origin, gr.VOXEL, gr.DIMS, gr.TRUNC)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(3)
    err = mgl.global_aligned_reconstruction_error(dev(moved), tf, tv, tf, thresholds=(0.01,), generator=gen,
                                                  **scene_kwargs(levels, origin))
    rot, tr = mr.pose_error(host(err["R"]), host(err["t"]), R_true, t_true)
    print("before: accuracy mean %.3f, within 0.01: %.3f; after: mean %.2e, within %.3f; pose %.4f degrees / %.2e" % (
        err["before"]["accuracy"]["mean"], err["before"]["accuracy"]["within"][0], err["accuracy"]["mean"],
        err["accuracy"]["within"][0], rot, tr))
    assert err["before"]["accuracy"]["mean"] > 10 * 0.01 and err["before"]["accuracy"]["within"][0] < 0.1
    assert err["accuracy"]["within"][0] == 1.0 and err["completeness"]["within"][0] == 1.0
    assert rot < MAX_ROT_DEG and tr < MAX_T
    assert set(err["starts"]) == {"R", "t", "score", "rot_index"} and err["starts"]["R"].shape == (gr.K_STARTS, 3, 3)
    assert {"R", "t", "icp", "before", "accuracy", "completeness", "chamfer", "fscore"} <= set(err)


@pytest.mark.parametrize("seed", gr.SCENE_SEEDS)
def test_global_mesh_icp_with_outliers(mgl, scene_levels, seed):
    """512 samples and 51 outliers uniform in the box, Tukey weights and rim rejection in the refinement.  The reference
    (tests/meshglobal_ref.global_mesh_icp with tests/meshrobust_ref.robust_mesh_icp, on the CPU) ends 0.055 degrees /
    1.8e-4, 0.013 / 4.2e-4 and 0.099 / 2.6e-4 from the truth on seeds 1, 2 and 3: all three meet the thresholds of
    tests/test_mesh_robust_host.py, seed 3 barely."""
    from tests.test_mesh_robust_host import MAX_ROT_DEG as ROBUST_ROT, MAX_T as ROBUST_T
    levels, origin = scene_levels
    sc = gr.make_scene(seed, outliers=0.1)
    assert len(sc["points"]) == 563
    R, t, info = mgl.global_mesh_icp(dev(sc["points"]), dev(sc["verts"]), dev(sc["faces"]),
                                     robust=dict(kernel="tukey", rim=True), **scene_kwargs(levels, origin))
    rot, tr = mr.pose_error(host(R), host(t), sc["R_true"], sc["t_true"])
    print("outliers, seed %d: %.4f degrees / %.2e, best %d, last scale %s" % (seed, rot, tr, int(info["best"]),
                                                                            host(info["icp"]["scale"][-1])))
    assert int(info["ok"][info["best"]]) == 1 and "scale" in info["icp"]
    assert rot < ROBUST_ROT and tr < ROBUST_T
